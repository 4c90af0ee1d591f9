// Arch.cpp — execution backend: turns queued stages into GPU launches through the C ABI.
#include "Arch.h"

#include <algorithm>
#include <chrono>
#include <fstream>
#include <iterator>
#include <cstring>
#include <set>

#include "Records.h"

#include "../../homulator_amd/csrc/hm_params.h"
#include "../../include/homulator_hip.h"

// the back-end's capability table for this ring size (hm_capability: host-side data, no GPU): which fused forms have kernels.  The fusion
// passes (Planner.cpp) and the launch builder ask it instead of naming ring sizes or digit widths (round 6).
uint32_t Arch::cap(uint32_t logN, const char *name) {
  uint64_t v = 0;
  return hm_capability(logN, name, &v) == HM_OK ? (uint32_t)v : 0u;
}

// one C-ABI call, with its argument arrays prebuilt so that run() is a tight loop of calls
struct Arch::Launch {
  enum Kind { L_NTT, L_INTT, L_EWE, L_BCONV, L_AUTO, L_NTT_SUBSCALE, L_TENSOR, L_EXCH_IN, L_EXCH_OUT, L_REPLICATE, L_IP, L_NTT_IP,
              L_BCONV_COL, L_EXCH_IN_COL, L_EXCH_OUT_COL,   // round 4: conversion + first pass on a rank's column slice, between the transposed-domain exchanges
              L_IP_HOISTED,                                  // (6h) the key products of several rotations from one set of digits
              L_IP_LINTRANS,                                 // (6l) ... and their plaintext-weighted sum
              L_TENSOR_DOT,                                  // (5d) the tensor products of several pairs of ciphertexts, summed
              L_IP_ROTSUM,                                   // (6s) the key products of rotations of different ciphertexts, summed
              L_IP_LINTRANS_MULTI,                           // (6m) several plaintext-weighted sums of the same hoisted key products
              L_TENSOR_SQUARE,                               // (5q) the scaled square of one ciphertext plus a constant
              L_LINCOMB,                                     // (5l) the sum of scaled polynomials plus a constant
              L_TENSOR_MULADD,                               // (5m) the scaled tensor product plus scaled addends plus a constant
              L_REIM,                                        // (5r) the sum and the rotated difference of a polynomial and its conjugate
              L_CLINCOMB,                                    // (5c) the sum of polynomials times a + b X^(N/2) plus a constant
              L_PLINCOMB,                                    // (5p) the sum of ciphertexts times plaintexts plus a plaintext on c0, both components
              L_TENSOR_DOTADD,                               // (5a) the scaled sum of tensor products plus scaled addends plus a constant
              L_LINCOMB_MULTI } kind;                        // (5L) several sums of scaled polynomials over the same inputs, each plus a constant
  std::vector<uint32_t> hoistG;   // L_IP_HOISTED: the Galois element of every rotation (a: digits [n][T], b: keys [r][n][2][T], out: [r][n][2])
                                  // L_IP_LINTRANS: the same, with c: plaintexts [r][n], d: addend source [n] / out1: addend output [n] (HM_NO_LIMB: none; both
                                  // empty: no entry has one), out: [n][2]
  Launch *xin = nullptr, *xout = nullptr;   // sharded BCONV: the exchange launches around it (they share its slice buffers)
  int recordSlot = -1;            // exchange launches of a pipelined sharded plan: the mark set behind them (hm_exchange_mark)
  std::vector<int> waitSlots;     // marks the compute stream waits for before this launch (hm_exchange_wait)
  std::vector<uint8_t> ipCoeff;   // L_NTT_IP: per (limb, digit) 1 = transformed inside the kernel (a = source, c = first-pass scratch)
  std::vector<uint8_t> ipInv;     // L_NTT_IP (7b): per limb, 1 = the outputs leave as the first pass of their inverse transform
  bool secondOnly = false;        // L_INTT (7b): hm_ntt_second_pass — the first pass was run by the inner-product kernel
  std::vector<uint8_t> outPacked; // L_INTT (11): per limb-poly, 1 = stored in the split-30 packed form of the conversions' inputs
  std::vector<uint32_t> inGalois, addGalois;   // (12) L_INTT: per limb-poly, the input / L_NTT_SUBSCALE: the addend is read through X -> X^g (0: as stored); empty: none
  std::vector<uint32_t> liftMods;              // L_NTT: per limb-poly, the modulus its stored input is reduced by; the transform lifts it into its own (hm_ntt_lift, ModRaise); empty: none
  std::vector<uint32_t> mulB;                  // (4p) L_INTT: the input, L_NTT_SUBSCALE: the minuend is the product with this limb-poly (hm_ntt_mul / hm_ntt_mix_sub_scale_mul); empty: none
  uint32_t xGalois = 0;                        // (12) L_NTT_IP: the evaluation-form digits, L_IP: the x operands are read through X -> X^g
  uint32_t ipTerms = 0, ipOuts = 0;
                                  // L_IP_ROTSUM: hoistG = the element of every ciphertext; a: digits [c][n][T], b: keys [c][n][2][T], d: addend sources
                                  // [c][n] / out1: addend output [n] (HM_NO_LIMB: none; both empty: no entry has one), out: [n][2]
                                  // L_IP_LINTRANS_MULTI: as L_IP_LINTRANS with multiOuts sums (L_IP_LINTRANS: 1): c: plaintexts [m][r][n], out: [m][n][2], out1: [m][n]
                                  // L_IP_ROTSUM with initial sums (hm_ip_rotsum_init_desc): c: init [n][2], d1: the initial addend sums [n]
                                  // ... with the identity step (hm_ip_lintrans_id_desc, either kind): idPt: identity plaintexts [m][n], d1: the second addend
                                  // source [n], out2: its outputs [m][n] (HM_NO_LIMB where d is); all empty: no identity step
  uint32_t multiOuts = 0;
  std::vector<uint32_t> idPt, d1;
  uint32_t dotTerms = 0;          // L_TENSOR_DOT: pairs per record (a, b, c, d: [n][dotTerms], roles as L_TENSOR; out, out1, out2: [n])
                                  // L_LINCOMB: terms per record (a: [n][dotTerms], out: [n]; k: the scalars [n][dotTerms], addK: the constants [n], empty: none)
                                  // L_LINCOMB_MULTI: terms per record and multiOuts sums (a: [n][dotTerms], out: [n][multiOuts]; k: the scalars
                                  // [n][multiOuts][dotTerms], addK: the constants [n][multiOuts], empty: none)
                                  // L_TENSOR_SQUARE: a = c0, c = c1, out, out1, out2 = d0, d1, d2 [n]; k: the scalars [n], addK: the constants [n] (empty: none)
                                  // L_REIM: a = the polynomial, c = its conjugate, out = the sum, out1 = the rotated difference [n]
                                  // L_CLINCOMB: as L_LINCOMB with k: the real parts a_t, maK: the monomial parts b_t [n][dotTerms]
                                  // L_PLINCOMB: terms per record (b: the plaintexts, x0, x1: c0, c1 of the ciphertexts [n][dotTerms]; d: the addend [n], empty:
                                  // none; out, out1: the sums of c0, c1 [n])
                                  // L_TENSOR_DOTADD: pairs per record (a, b, c, d: [n][dotTerms]) and maAddends addends (x0, x1: [n][maAddends]); out, out1, out2 [n];
                                  // k: the pair scalars [n][dotTerms] (empty: none), maK: the addend scalars [n][maAddends], addK: the constants [n] (empty: none)
  uint32_t maAddends = 0;         // L_TENSOR_MULADD: addends per record (a, b, c, d, out, out1, out2 as L_TENSOR; x0, x1: c0, c1 of the addends [n][maAddends];
  std::vector<uint32_t> x0, x1;   // k: the scalars [n], maK: the addend scalars [n][maAddends], addK: the constants [n]; k / addK empty: none)
  std::vector<uint64_t> maK;
  std::string name;
  std::string statKey;
  int opcode = 0;
  uint32_t galois = 0;
  std::vector<uint32_t> a, b, c, d, out, out1, out2, mods, inMods;
  struct Prob { std::vector<uint32_t> in, inMods, out, outMods, epA, epB; std::vector<uint64_t> epK; bool epi = false, epAdd = false, inPacked = false; };
  std::vector<Prob> probs;  // BCONV: independent conversions batched into one launch
  // multi-GPU: exchange steps (limb list + owner of each limb) and the coefficient-slice buffers of a sharded BCONV
  std::vector<uint32_t> exLimbs, exOwners;
  uint64_t *slicesIn = nullptr, *slicesOut = nullptr;
  uint32_t logLen = 0;
  std::vector<uint64_t> k, mixK, addK;  // mixK / addK: prologue and addend constants of the merged ModDown + rescale transform
  bool hasK = false;
  unsigned long long refInstructions = 0;
  unsigned long long bytes = 0;  // operand limb-polys read + written x N x 8
};

static hm::Params &hostP(void *p) { return *static_cast<hm::Params *>(p); }

Arch::Arch(Config *cfg) : config(cfg) {
  n = cfg->getValue("N");
  logN = 0;
  while ((1u << logN) < n) ++logN;
  clusterCount = cfg->getValueOr("cluster", 1);
  uint32_t b = cfg->getValueOr("backend", BACKEND_HIP);
  if (const char *e = getenv("HOMULATOR_BACKEND")) b = std::string(e) == "count" ? BACKEND_COUNT : std::string(e) == "sim" ? BACKEND_SIM : BACKEND_HIP;
  backendKind = b == BACKEND_COUNT ? BACKEND_COUNT : b == BACKEND_SIM ? BACKEND_SIM : BACKEND_HIP;
  world_ = cfg->getValueOr("world", 0);
  rank_ = cfg->getValueOr("rank", 0);
  if (world_ == 0) {
    // no explicit `world` key: one rank per GPU when started by a multi-process launcher (torch.distributed.run, mpirun
    // wrappers: WORLD_SIZE / RANK / LOCAL_RANK).  The CLI's [cluster] argument doubles as the GPU count:
    // when it was given on the command line it must agree with the launcher.
    world_ = 1;
    const char *ws = getenv("WORLD_SIZE"), *rk = getenv("RANK"), *lr = getenv("LOCAL_RANK");
    // ... and only for the CLI (it sets `launcher_env`): a library user who builds an op inside a torchrun job without saying
    // `world` gets a plain one-GPU op on the device they asked for, not a silently sharded one on LOCAL_RANK
    if (ws && atoi(ws) > 1 && b == BACKEND_HIP && cfg->getValueOr("launcher_env", 0)) {
      world_ = (uint32_t)atoi(ws);
      rank_ = rk ? (uint32_t)atoi(rk) : 0;
      if (lr && !getenv("HOMULATOR_DEVICE") && !cfg->hasKey("device")) cfg->setValue("device", (uint32_t)atoi(lr));
      if (cfg->getValueOr("cluster_from_argv", 0) && clusterCount != world_)
        throw std::runtime_error("[cluster] = " + std::to_string(clusterCount) + " GPUs requested, but the launcher started " + std::to_string(world_) + " ranks");
    }
  }
  if (rank_ >= world_) throw std::runtime_error("rank must be below world");
  if (world_ & (world_ - 1)) throw std::runtime_error("world must be a power of two");
  // HIP-graph replay of the whole plan: no gain in steady state (the op is GPU-bound), but the host prepares a launch set in ~20 us instead of
  // ~0.3 ms: +3-5 % on a 20-step timed region of batched instances (bench.py turns it on for them), -4 % one op at a time (replay overhead)
  useGraph = cfg->getValueOr("graph", 0) != 0;
  if (const char *e = getenv("HOMULATOR_GRAPH")) useGraph = std::string(e) != "0";
  batch_ = std::max<uint32_t>(1, cfg->getValueOr("batch", 1));
  if (const char *e = getenv("HOMULATOR_BATCH")) batch_ = std::max(1, atoi(e));
  fuse = cfg->getValueOr("fuse", 1) != 0;
  if (const char *e = getenv("HOMULATOR_FUSE")) fuse = std::string(e) != "0";
  // the HPIP unit as a fused NTT-epilogue x evaluation-key MAC.  Upstream switches its HPIP unit with
  // `hasHPIPU` (src/Arch.cpp:10; 0 in the shipped files, where the inner product runs on the EWE); that key keeps describing
  // the SIMULATED machine (backend = sim).  On the GPU the fused kernel is a scheduling decision of the backend: `fuse_hpip`.
  fuseHpip = cfg->getValueOr("fuse_hpip", 1) != 0;
  if (const char *e = getenv("HOMULATOR_FUSE_HPIP")) fuseHpip = std::string(e) != "0";
  // ... and the ModUp base conversion inside the first pass of that transform (BConvOut_(j) never reaches HBM): N = 2^16, up to 15
  // input limbs per digit, one GPU (a sharded conversion works on coefficient slices)
  fuseBconv = cfg->getValueOr("fuse_bconv", 1) != 0;
  if (const char *e = getenv("HOMULATOR_FUSE_BCONV")) fuseBconv = std::string(e) != "0";
  // ... and the ModDown conversion inside the first pass of the merged ModDown + rescale transform (round 4, pass 9): built, bit-exact, and
  // measured SLOWER on MI355X in both modes (profiles/r04_fuse_ab.txt: batch 10 conversion 18.5 + transform 51.7 us per op against 3.6 + 70.8
  // fused; one at a time 24.9 + 70.5 against 9.5 + 89.2): the separate conversion kernel converts to all 35 outputs of a key from inputs it
  // loads and splits ONCE, the fused form loads the 15 input tiles again for every pair of outputs, and the 73 MB of ModdownBConvOut traffic it
  // saves is worth less than that.  Opt-in (config key fuse_moddown = 1).
  // (7b, round 5) InnerProOut -> ModDownINTTOut (src/Operation.cpp:294-445): the special limbs of the key-switch sum are read by nothing but
  // the ModDown's inverse transform, whose first pass is a ROW pass over the 16 rows the inner-product workgroup already owns: the kernel
  // runs it on its accumulators and the INTT launch keeps the COL pass.  N = 2^16, one GPU.  Config key fuse_ip_inv (default 1).
  fuseIpInv = cfg->getValueOr("fuse_ip_inv", 1) != 0;
  if (const char *e = getenv("HOMULATOR_FUSE_IP_INV")) fuseIpInv = std::string(e) != "0";
  // (11, round 5) the inverse transforms whose outputs are read by base conversions only (ModUp_DecompOut, ModDownBConvStep1) store them in
  // the split-30 packed form the conversions multiply with: two instructions per value in the producer instead of two per value and reading
  // workgroup (18 per value in a 35-output ModUp digit).  Config key pack_bconv_in (default 1).
  packBconvIn = cfg->getValueOr("pack_bconv_in", 1) != 0;
  if (const char *e = getenv("HOMULATOR_PACK_BCONV_IN")) packBconvIn = std::string(e) != "0";
  // (12, round 6) an automorphism whose output only feeds inverse transforms' inputs / fused forward transforms' addends is read through by them
  // (hrotate: AUTO_Key(0) -> the final add).  Config key fuse_auto (default 1).
  fuseAuto = cfg->getValueOr("fuse_auto", 1) != 0;
  if (const char *e = getenv("HOMULATOR_FUSE_AUTO")) fuseAuto = std::string(e) != "0";
  fuseModDown = cfg->getValueOr("fuse_moddown", 0) != 0;
  if (const char *e = getenv("HOMULATOR_FUSE_MODDOWN")) fuseModDown = std::string(e) != "0";
  // (6h) hrotate_hoisted: the R key products over automorphisms of the same digits become one hm_inner_product_hoisted launch.  Config key
  // fuse_hoist (default 1).
  fuseHoist = cfg->getValueOr("fuse_hoist", 1) != 0;
  // (6l) hlintrans: those key products, the plaintext products and the sums over the rotations become one hm_inner_product_lintrans launch.
  // Config key fuse_lintrans (default 1).
  fuseLintrans = cfg->getValueOr("fuse_lintrans", 1) != 0;
  // (5d) hdot: the tensor product of pair 1 and the multiply-accumulate chains of the further pairs become one hm_tensor_dot launch.  Config key
  // fuse_dot (default 1).
  fuseDot = cfg->getValueOr("fuse_dot", 1) != 0;
  // (5q) hsquare: the tensor product of the ciphertext with itself, the scalar on its three outputs and the constant on d0 become one
  // hm_tensor_square launch.  Config key fuse_square (default 1).
  fuseSquare = cfg->getValueOr("fuse_square", 1) != 0;
  // (5l) hlincomb: the MUL_CONST of every term, the ADDs between them and the ADD_CONST behind them become one hm_lincomb launch.  Config key
  // fuse_lincomb (default 1).
  fuseLincomb = cfg->getValueOr("fuse_lincomb", 1) != 0;
  // (5m) hmuladd: the tensor product, the scalar on its three outputs, the MUL_CONST + ADD pairs of the addends on d0 and d1 and the constant on d0
  // become one hm_tensor_muladd launch.  Config key fuse_muladd (default 1).
  fuseMuladd = cfg->getValueOr("fuse_muladd", 1) != 0;
  // (5r) hreim: the ADD, the SUB and the MUL by the evaluation form of -X^(N/2) behind the conjugation become one hm_reim_split launch.  Config key
  // fuse_reim (default 1).
  fuseReim = cfg->getValueOr("fuse_reim", 1) != 0;
  // (5c) hclincomb: per term the MUL_CONST, the MUL by the evaluation form of -X^(N/2) with its MUL_CONST and the ADD of both, the ADDs between the
  // terms and the ADD_CONST behind them become one hm_clincomb launch.  Config key fuse_clincomb (default 1).
  fuseClincomb = cfg->getValueOr("fuse_clincomb", 1) != 0;
  // (5p) hplincomb: the MUL and the MAC_ADDs of both components and the ADD of the plaintext addend become one hm_plincomb launch.  Config key
  // fuse_plincomb (default 1).
  fusePlincomb = cfg->getValueOr("fuse_plincomb", 1) != 0;
  // (5a) hdotadd: the tensor products of all pairs, the scalars on their outputs, the ADDs between the pairs, the MUL_CONST + ADD pairs of the
  // addends on d0 and d1 and the constant on d0 become one hm_tensor_dotadd launch.  Config key fuse_dotadd (default 1).
  fuseDotadd = cfg->getValueOr("fuse_dotadd", 1) != 0;
  // (5L) hmlincomb: the (5l) records over one list of inputs become one record of ONE hm_lincomb_multi launch.  Config key fuse_mlincomb
  // (default 1); 0 leaves them to (5l)'s launch
  fuseMlincomb = cfg->getValueOr("fuse_mlincomb", 1) != 0;
  // (4p) pmult with rescale = 1: the products are formed by the rescale's transforms while they load.  Config key fuse_pmul_rescale: 1 / 0 = always /
  // never; not given = where it was measured faster than the three-launch plan: everywhere but the generic back-end's launches
  // inside the one-launch form's limit, which has no product form there (Planner::productOperands)
  fusePmulRescale = cfg->getValueOr("fuse_pmul_rescale", 1) != 0;
  fusePmulAuto = !cfg->hasKey("fuse_pmul_rescale");
  genericArith = cfg->getValueOr("chain_bits", 0) != 0;
  // (6s) hrotsum: the key products of rotations of different ciphertexts, the sums over the ciphertexts and the rotated c0's become one
  // hm_inner_product_rotsum launch.  Config key fuse_rotsum (default 1).
  fuseRotsum = cfg->getValueOr("fuse_rotsum", 1) != 0;
  // (6m) hbsgs: the key products of the baby rotations and the M >= 2 weighted sums over them become one hm_inner_product_lintrans_multi launch.
  // Config key fuse_bsgs (default 1).
  fuseBsgs = cfg->getValueOr("fuse_bsgs", 1) != 0;
  // sharded runs: the exchanges of digit j+1 run on the context's exchange stream while digit j converts and transforms (SURVEY.md 7:
  // 2 beta + 2 all-to-alls per key switch instead of 4, same order on every rank).  The per-digit transforms must then stay separate
  // launches, so the fused NTT x key kernel (which needs all digits) is not used.
  pipelineDigits = world_ > 1 && cfg->getValueOr("pipeline_digits", 1) != 0;
  if (const char *e = getenv("HOMULATOR_PIPELINE_DIGITS")) pipelineDigits = world_ > 1 && std::string(e) != "0";
  // round 4: the fused kernels serve the sharded plan too — the ModUp conversion AND the first pass of its transforms run on the slice
  // holder's COLUMN slice (exchange in the transposed domain), the limb owner runs the transform x key kernel's second pass (config key
  // shard_fused, default 1; needs world <= the column tiles of a limb-poly the back-end deals out: cap_col_slices).  Otherwise the per-digit transforms stay launches of their own.
  shardFused = world_ > 1 && cfg->getValueOr("shard_fused", 1) != 0 && fuseHpip && fuseBconv && world_ <= cap(logN, "cap_col_slices");
  if (const char *e = getenv("HOMULATOR_SHARD_FUSED")) shardFused = shardFused && std::string(e) != "0";
  // Round 5: a second sharded plan, chosen by the bytes it moves.  `gather`: the conversions' INPUT limbs (the l scaled
  // limbs of the ModUp, the 2 alpha of the ModDown) are replicated to every rank (hm_replicate_limbs: one collective each) and every rank
  // runs the ONE-GPU kernels — conversion inside the first pass, transform x key — for the output limbs it owns: per-rank ingress
  // (l + 2 alpha)(G - 1) / G limb-polys against (2 beta E + 2 alpha)(G - 1) / G^2 for the all-to-all pair around every conversion: half the
  // bytes at G = 2, the same at G = 4, twice at G = 8 — and 3 collectives per key switch instead of 2 beta + 3.  The links are point to
  // point (one 77 GB/s link per pair and direction), so at G <= 4 the bytes decide.  Config key shard_plan: 0 = by rank count (gather up to 4
  // ranks, all-to-all above), 1 = all-to-all (the transposed-domain plan of round 4), 2 = gather.
  {
    uint32_t plan = cfg->getValueOr("shard_plan", 0);
    if (const char *e = getenv("HOMULATOR_SHARD_PLAN")) plan = (uint32_t)atoi(e);
    shardGather = world_ > 1 && (plan == 2 || (plan == 0 && world_ <= 4));
    if (shardGather) { shardFused = false; pipelineDigits = false; }
  }
  if (pipelineDigits && !shardFused) fuseHpip = false;
  stat = new Statistic();
}

Arch::~Arch() {
  if (graph) hm_graph_destroy(static_cast<hm_graph *>(graph));
  if (ctx)
    for (void *p : sliceBuffers) hm_free(ctx, p);
  if (ctx)
    for (auto &kv : snapshots) hm_free(ctx, kv.second.first);
  if (ctx && encodeScratch) hm_free(ctx, encodeScratch);
  if (ctx) {
    if (pool) hm_free(ctx, pool);
    hm_destroy(ctx);
  }
  delete static_cast<hm::Params *>(hostParams);
  delete stat;
  delete sim;
}

void Arch::loadSim(SimProgram &&program) {
  if (backendKind != BACKEND_SIM) throw std::runtime_error("loadSim: backend is not sim");
  delete sim;
  sim = nullptr;
  sim = new SimModel(config, std::move(program));
}

void Arch::commInitRccl(const void *id) {
  if (!ctx) throw std::runtime_error("commInitRccl: no HIP context");
  if (hm_comm_init_rccl(ctx, (int)rank_, (int)world_, id) != HM_OK) throw std::runtime_error(std::string("hm_comm_init_rccl: ") + hm_last_error(ctx));
  commReady = true;
}
void Arch::commInitExternal(void *fn, void *user) {
  if (!ctx) throw std::runtime_error("commInitExternal: no HIP context");
  if (hm_comm_init_external(ctx, (int)rank_, (int)world_, reinterpret_cast<hm_exchange_fn>(fn), user) != HM_OK)
    throw std::runtime_error(std::string("hm_comm_init_external: ") + hm_last_error(ctx));
  commReady = true;
}

void Arch::bindParams(uint32_t maxLevel, uint32_t curLevel, uint32_t alpha) {
  maxLevel_ = maxLevel;
  curLevel_ = curLevel;
  if (hostParams) return;
  hm::Params *hp = new hm::Params;
  // config key `chain_bits` (build-specific; the reference pins no modulus): 0 = the default chain (primes h 2^32 + 1 below 2^60: the
  // word-wise Montgomery back-end); b in [21, 60] = the maxLevel + alpha largest primes = 1 mod 2N below 2^b — 60 is SURVEY.md 8(d)'s
  // chain as written, 36 a chain of 36-bit words as upstream's `elementBitWidth` models (config/config_4.cfg:9).  hm_create picks the
  // arithmetic back-end from the chain it is handed.
  const uint32_t chainBits = config->getValueOr("chain_bits", 0);
  std::vector<uint64_t> chain;
  if (chainBits) chain = hm::Params::chain_below(logN, chainBits, maxLevel + alpha);
  const uint64_t *cq = chainBits ? chain.data() : nullptr, *cp = chainBits ? chain.data() + maxLevel : nullptr;
  hp->init(logN, maxLevel, alpha, cq, cp, nullptr, /*forGeneric: the host side only needs moduli and conversion constants*/ chainBits != 0);
  hostParams = hp;
  if (backendKind == BACKEND_HIP) {
    hm_params p = {logN, maxLevel, alpha, (int32_t)config->getValueOr("device", 0), cq, cp, nullptr};
    if (const char *e = getenv("HOMULATOR_DEVICE")) p.device = atoi(e);
    if (hm_create(&ctx, &p) != HM_OK)
      throw std::runtime_error(std::string("HIP backend unavailable: ") + hm_last_error(nullptr));
  }
}

uint64_t Arch::modulus(uint32_t modId) const { return hostP(hostParams).mod.at(modId); }

std::vector<uint64_t> Arch::bconvScale(const std::vector<uint32_t> &inMods) {
  std::vector<uint64_t> qh(inMods.size()), tb(inMods.size());
  hostP(hostParams).bconv_consts(inMods.data(), (uint32_t)inMods.size(), nullptr, 0, qh.data(), tb.data());
  return qh;
}

void Arch::registerLimbs(const std::vector<AddrType> &limbStarts) {
  for (AddrType a : limbStarts)
    if (!limbIndex.count(a)) {
      uint32_t idx = (uint32_t)limbIndex.size();
      limbIndex[a] = idx;
    }
}

uint32_t Arch::limbOf(AddrType a) const {
  auto it = limbIndex.find(a);
  if (it == limbIndex.end()) throw std::runtime_error("address " + std::to_string(a) + " is not a registered limb");
  return it->second;
}

void Arch::bindInput(const std::vector<AddrType> &dst, Arch *src, const std::vector<AddrType> &srcAddrs) {
  if (prepared) throw std::runtime_error("bindInput after prepare()");
  if (!src || src == this) throw std::runtime_error("bindInput: bad producer");
  if (dst.size() != srcAddrs.size()) throw std::runtime_error("bindInput: " + std::to_string(srcAddrs.size()) + " limb-polys produced, " + std::to_string(dst.size()) + " expected (levels differ)");
  if (src->n != n || src->batch_ != batch_ || src->world_ != world_ || src->rank_ != rank_ || src->backendKind != backendKind)
    throw std::runtime_error("bindInput: producer and consumer differ in N, batch, sharding or backend");
  bindings.push_back(Binding{dst, src, srcAddrs, {}, {}, {}});
}

void Arch::issueIns(uint32_t, const std::string &, const Stage &stage) {
  if (prepared) throw std::runtime_error("issueIns after prepare()");
  stages.push_back(stage);
}
void Arch::issueIns(uint32_t index, const std::string &name, std::vector<Instruction *> &insg) {
  if (insg.empty()) return;
  Stage st;
  st.name = name + "_" + std::to_string(stages.size());
  st.kind = insg[0]->ops;
  st.ins = insg;
  st.cluster0 = index;
  issueIns(index, name, st);
}
void Arch::issueIns(uint32_t index, uint32_t h, uint32_t w, std::vector<Instruction *> &insg, bool hpip) {
  if (h == 0 && w == 0) issueIns(index, hpip ? "HPIP" : "BCONV", insg);
}

// ---------------------------------------------------------------------------------------------------
// stage -> launch.  Arch::buildLaunches (at the end of this section) splits the stages into parts one C-ABI call can express, gives every
// part its dependency depth, and hands every (depth, key) group to LaunchBuilder, which has one emit function per launch kind.
// ---------------------------------------------------------------------------------------------------
namespace {
struct Part { std::string name; int key; std::vector<Instruction *> ins; int depth = 0; };
typedef std::vector<const Part *> Group;

// records of one stage with equal keys go into one C-ABI call (same kind / opcode / direction / operand shape)
int partKey(const Instruction &i) {
  if (!i.ipSumX.empty()) return 9000 + (int)i.ipX.size() * 100 + (int)i.ipSumX.size();                     // 9000+: sum of rotations of different ciphertexts, by digits and ciphertexts
  if (i.ipLinPt.size() > 1) return 10000 + (int)i.ipX.size() * 400 + ((int)i.ipHoistG.size() - 1) * 17 + (int)i.ipLinPt.size();   // 10000+: several weighted sums, by digits, rotations and groups
  if (!i.ipLinPt.empty()) return 7000 + (int)i.ipX.size() * 100 + (int)i.ipHoistG.size();                  // 7000+: weighted sum of hoisted key products, by digits and rotations
  if (i.ipHoistG.size() == 1) return 20000 + (int)i.ipX.size() + 8 * (int)i.ipHoistG[0];                   // 20000+: hoisted key product of ONE rotation, by digits and element (hrotsum with fuse_rotsum = 0: one per ciphertext)
  if (!i.ipHoistG.empty()) return 6000 + (int)i.ipX.size() * 100 + (int)i.ipHoistG.size();                 // 6000+: hoisted key product, by digits and rotations
  if (i.ops == IP && transformsInside(i)) return 400 + (int)i.ipX.size() * 10 + (int)i.ipY.size();         // 400+: transform x key, by digits and keys
  if (isKeyProduct(i)) return 300 + (int)i.ipX.size() * 10 + (int)i.ipY.size();                            // 300+: key product, by digits and keys
  const Fused &f = i.fu;
  switch (f.form) {
    case FusedForm::None: break;
    case FusedForm::TensorDot: return 8000 + (int)f.terms;                                                  // 8000+: sum of tensor products, by pairs
    case FusedForm::Square: return 8500 + (f.hasScale ? 1 : 0) + (f.hasConst ? 2 : 0);                      // 8500+: scaled square plus constant, by what it absorbed
    case FusedForm::LincombMulti: return 12000 + 16 * ((int)f.terms - 1) + (int)f.rowScales.size() - 1;     // 12000+: several sums of scaled polynomials, by terms and sums (12000 .. 12255)
    case FusedForm::Lincomb: return 8600 + (int)f.terms;                                                    // 8600+: sum of scaled polynomials, by terms
    case FusedForm::MulAdd: return 8700 + 4 * (int)f.addends + (f.hasScale ? 1 : 0) + (f.hasConst ? 2 : 0); // 8700+: scaled product plus addends, by addends and what it absorbed
    case FusedForm::DotAdd: return 8100 + 9 * ((int)f.terms - 1) + (int)f.addends;                          // 8100+: scaled sum of products plus addends, by pairs and addends (8100 .. 8243)
    case FusedForm::ReIm: return 8400;                                                                      // 8400: sum and rotated difference of a polynomial and its conjugate
    case FusedForm::CLincomb: return 8800 + (int)f.terms;                                                   // 8800+: sum of polynomials times a + b X^(N/2), by terms
    case FusedForm::PLincomb: return 8900 + 2 * (int)f.terms + (f.hasAddend ? 1 : 0);                       // 8900+: sum of ciphertexts times plaintexts, by terms and addend
  }
  if (i.fusedTensor) return 200;                                                                           // 200: tensor product
  if (i.fusedSubScale && i.fMinuendB) return i.fMix ? 211 : 209;                                           // 209 / 211: ... with a product minuend (4p)
  if (i.fusedSubScale) return (i.fMix ? 203 : 201) + (i.fConvIn.empty() ? 0 : 4);                          // 201 / 203: fused forward transform, plain / merged; 205 / 207: with its conversion
  if (i.ops == MULT) return 100 + i.opcode;                                                                // 100+: element-wise, by opcode
  if (i.ops == NTT && i.passthrough) return 100 + EWE_COPY;                                                //       (unfused: a pass-through transform is a copy)
  if (i.ops == AUTO) return 1000 + (int)i.galois;                                                          // 1000+: automorphism, by element
  if (i.ops == NTT && i.liftSrcMod != kNoLift) return 5700;                                                // 5700: forward transform of a lifted input (ModRaise): never with plain ones
  return (int)i.ops + (i.secondOnly ? 5000 : 0) + (i.inMulB ? 5500 : 0);                                   // below 100: by op; 5000+: second pass only (7b); 5500+: product input (4p)
}

// what the kernels of a record load: a fused conversion REPLACES the address it would have written (the passes count that one too)
std::vector<AddrType> loads(const Instruction &i) {
  std::vector<AddrType> v;
  for (const Read &r : recordReads(i))
    if (r.loaded()) v.push_back(r.addr);
  return v;
}

// dependency depth of every part (RAW, WAR and WAW through limb addresses).  With fuse = 1 parts of equal depth and kind are coalesced
// into one launch: the two keys of a ModDown, the beta digits of a ModUp, D0/D2 of the tensor product ...  The reference dispatches stage
// by stage (Operation.cpp:947-964); the stage ORDER it fixes is only a topological order of this graph.
void assignDepths(std::vector<Part> &parts, bool fuse) {
  std::map<AddrType, int> writerDepth, readerDepth;
  int serial = 0;
  for (Part &p : parts) {
    int d = 0;
    for (Instruction *i : p.ins) {
      for (AddrType a : loads(*i)) { auto w = writerDepth.find(a); if (w != writerDepth.end()) d = std::max(d, w->second + 1); }
      for (const Write &o : recordWrites(*i)) {
        auto w = writerDepth.find(o.addr); if (w != writerDepth.end()) d = std::max(d, w->second + 1);
        auto r = readerDepth.find(o.addr); if (r != readerDepth.end()) d = std::max(d, r->second + 1);
      }
    }
    if (!fuse) d = serial++;  // unfused: one launch per stage part, upstream's order
    p.depth = d;
    for (Instruction *i : p.ins) {
      for (AddrType a : loads(*i)) { int &r = readerDepth[a]; r = std::max(r, d); }
      for (const Write &o : recordWrites(*i)) writerDepth[o.addr] = d;
    }
  }
}

// One GPU runs its launches on ONE in-order stream, and the launches of a level go out in the order of the first part of every key.  A part one
// level below a group of its own key may therefore join that group when every part of the group's level it conflicts with (RAW, WAR, WAW) is
// launched in FRONT of the group: the stream orders them.  (hsquare with fuse_square = 0: the constant lands on d0 one launch behind the scalar
// that ModUp's inverse transforms wait for; the inverse transform of d0's last limb joins them instead of running as a launch of one limb-poly.)
void addUnique(std::vector<int> &v, int x);
void joinEarlierGroups(std::vector<Part> &parts) {
  struct Touched { std::set<AddrType> reads, writes; };
  std::vector<Touched> t(parts.size());
  int maxDepth = 0;
  for (size_t p = 0; p < parts.size(); ++p) {
    maxDepth = std::max(maxDepth, parts[p].depth);
    for (Instruction *i : parts[p].ins) {
      for (AddrType a : loads(*i)) t[p].reads.insert(a);
      for (const Write &o : recordWrites(*i)) t[p].writes.insert(o.addr);
    }
  }
  auto conflict = [&](size_t x, size_t y) {
    for (AddrType a : t[x].writes)
      if (t[y].reads.count(a) || t[y].writes.count(a)) return true;
    for (AddrType a : t[x].reads)
      if (t[y].writes.count(a)) return true;
    return false;
  };
  for (int d = 0; d < maxDepth; ++d) {
    std::vector<int> keys;   // the launch order of level d
    for (const Part &p : parts)
      if (p.depth == d) addUnique(keys, p.key);
    auto pos = [&](int key) { return (int)(std::find(keys.begin(), keys.end(), key) - keys.begin()); };
    for (size_t p = 0; p < parts.size(); ++p) {
      if (parts[p].depth != d + 1 || pos(parts[p].key) == (int)keys.size()) continue;
      bool ordered = true;
      for (size_t r = 0; r < parts.size() && ordered; ++r)
        if (r != p && parts[r].depth == d && pos(parts[r].key) >= pos(parts[p].key) && conflict(r, p)) ordered = false;
      if (ordered) parts[p].depth = d;
    }
  }
}

std::vector<Instruction *> flatten(const Group &group) {
  std::vector<Instruction *> recs;
  for (const Part *g : group) recs.insert(recs.end(), g->ins.begin(), g->ins.end());
  return recs;
}
void addUnique(std::vector<int> &v, int x) { if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x); }
}  // namespace

struct Arch::LaunchBuilder {
  typedef std::unique_ptr<Launch> LaunchPtr;
  typedef std::vector<LaunchPtr> Launches;
  typedef const std::vector<Instruction *> &Recs;
  Arch &A;
  const unsigned long long LP;            // bytes of a limb-poly
  const unsigned long long bconvPorts;    // upstream issues every BCONV group to all MAC ports (include/Driver.h:307-320): same accounting here
  std::map<AddrType, uint32_t> ownerOfAddr;   // multi-GPU: who holds each limb-poly
  std::map<AddrType, int> slotOfAddr;         // pipelined sharded plan: the exchange mark behind which an address is valid on this rank
  int nextSlot = 0;

  explicit LaunchBuilder(Arch &a)
      : A(a), LP((unsigned long long)a.n * 8), bconvPorts((unsigned long long)a.config->getValueOr("bconv_num_high", 1) * a.config->getValueOr("bconv_num_width", 1)) {}

  uint32_t limb(AddrType a) const { return A.limbOf(a); }
  std::vector<uint32_t> limbs(const std::vector<AddrType> &v) const {
    std::vector<uint32_t> o;
    for (AddrType a : v) o.push_back(limb(a));
    return o;
  }
  bool mine(const Instruction *i) const { return A.owner(i->mod_id) == A.rank_; }
  void append(Launches &v) { for (LaunchPtr &l : v) A.launches.push_back(std::move(l)); }
  // the conversion of a launch with these inputs and flags, created behind the others if there is none yet (the order of `probs` is the order
  // of the kernel's work)
  static Launch::Prob &findOrAddProb(Launch &L, const std::vector<uint32_t> &in, const std::vector<uint32_t> &inMods, bool inPacked, bool epi = false,
                                     bool epAdd = false, bool *added = nullptr) {
    if (added) *added = false;
    for (auto &q : L.probs)
      if (q.in == in && q.inMods == inMods && q.epi == epi && q.epAdd == epAdd && q.inPacked == inPacked) return q;
    L.probs.push_back(Launch::Prob{in, inMods, {}, {}});
    L.probs.back().epi = epi; L.probs.back().epAdd = epAdd; L.probs.back().inPacked = inPacked;
    if (added) *added = true;
    return L.probs.back();
  }
  // keys, outputs and modulus of a key-product record; (12) a launch reads its evaluation-form digits through ONE automorphism: the records
  // that have such a digit must agree on it (0 = as stored counts), a record without one must not ask for any
  void keyProductRecord(Launch &L, const Instruction *i) {
    for (auto &y : i->ipY) for (AddrType yy : y) L.b.push_back(limb(yy));
    L.out.push_back(limb(i->OutputOperand));
    for (AddrType o : i->extraOutputs) L.out.push_back(limb(o));
    L.mods.push_back(i->mod_id);
    const bool evalDigit = i->ipCoeff.empty() || std::find(i->ipCoeff.begin(), i->ipCoeff.end(), 0) != i->ipCoeff.end();
    if (evalDigit ? (xGaloisSet && L.xGalois != i->ipXGalois) : i->ipXGalois != 0)
      throw std::runtime_error("key product: the records of one launch read their digits through different automorphisms");
    if (evalDigit) { L.xGalois = i->ipXGalois; xGaloisSet = true; }
  }
  bool xGaloisSet = false;   // ... of the launch being built
  // what the key products over the rotations of one launch share (the records must agree on the rotations): moduli, keys b [r][n][2][T] and the
  // digits, a [n][T], or with digitsPerRotation (6s: every rotation is of a ciphertext of its own) a [r][n][T].  Returns the number of rotations
  size_t hoistedOperands(Launch &L, Recs recs, const char *what, bool digitsPerRotation = false) {
    L.statKey = "EWE";
    L.ipTerms = (uint32_t)recs[0]->ipX.size(); L.ipOuts = 2; L.hoistG = recs[0]->ipHoistG;
    for (Instruction *i : recs) {
      if (i->ipHoistG != L.hoistG) throw std::runtime_error(std::string(what) + ": the records of one launch rotate by different elements");
      if (!digitsPerRotation) for (AddrType x : i->ipX) L.a.push_back(limb(x));
      L.mods.push_back(i->mod_id);
    }
    for (size_t r = 0; r < L.hoistG.size(); ++r)
      for (Instruction *i : recs) {
        if (digitsPerRotation) for (AddrType x : i->ipSumX[r]) L.a.push_back(limb(x));
        for (size_t k = 0; k < 2; ++k)
          for (AddrType y : i->ipY[r * 2 + k]) L.b.push_back(limb(y));
      }
    return L.hoistG.size();
  }

  void emitGroup(Group group);
  void shardedTransformTimesKey(const Group &group);
  void replicateForeignOperands(const Group &group);
  std::set<int> slotsOf(const Part *g) const;
  std::vector<Group> splitByExchangeMark(const Group &group) const;
  void emitCompute(const Group &group, Launches &front, Launches &back);
  void wrapShardedConversion(LaunchPtr L, Recs recs, Launches &front, Launches &back);
  void ipHoisted(Launch &L, Recs recs);
  void ipLintrans(Launch &L, Recs recs);
  void ipRotsum(Launch &L, Recs recs);
  void nttIp(Launch &L, Recs recs);
  void ip(Launch &L, Recs recs);
  void tensor(Launch &L, Recs recs);
  void tensorOutputs(Launch &L, const Instruction *i);
  void tensorSquare(Launch &L, Recs recs);
  void lincomb(Launch &L, Recs recs);        // (5l) and (5c)
  void lincombMulti(Launch &L, Recs recs);
  void tensorMulAdd(Launch &L, Recs recs);
  void reim(Launch &L, Recs recs);
  void plincomb(Launch &L, Recs recs);
  void tensorDotAdd(Launch &L, Recs recs);   // (5a) and (5d)
  void nttSubScale(Launch &L, Recs recs);
  void copy(Launch &L, Recs recs);
  void transform(Launch &L, Recs recs);
  void automorphism(Launch &L, Recs recs);
  void ewe(Launch &L, Recs recs);
  void bconv(Launch &L, Recs recs);
};

// (6h) one hoisted key product: digits a [n][T], keys b [r][n][2][T], outputs out [r][n][2] (hm_ip_hoisted_desc)
void Arch::LaunchBuilder::ipHoisted(Launch &L, Recs recs) {
  L.kind = Launch::L_IP_HOISTED;
  const size_t R = hoistedOperands(L, recs, "hoisted key product");
  for (size_t r = 0; r < R; ++r)
    for (Instruction *i : recs)
      for (size_t k = 0; k < 2; ++k) L.out.push_back(limb(r == 0 && k == 0 ? i->OutputOperand : i->extraOutputs[r * 2 + k - 1]));
  // digits read once, keys read and outputs written once per rotation
  L.bytes = (unsigned long long)recs.size() * (L.ipTerms + 2 * R * L.ipTerms + 2 * R) * LP;
}

// (6l, 6m) M weighted sums of the same hoisted key products: the hoisted launch's digits and keys, plaintexts c [m][r][n], outputs out [m][n][2];
// entries with an addend: source d [n], outputs out1 [m][n] (M = 1: hm_ip_lintrans_desc, else hm_ip_lintrans_multi_desc)
void Arch::LaunchBuilder::ipLintrans(Launch &L, Recs recs) {
  const size_t M = recs[0]->ipLinPt.size();
  const std::string what = M == 1 ? "weighted rotations" : "weighted rotations (several sums)";
  L.kind = M == 1 ? Launch::L_IP_LINTRANS : Launch::L_IP_LINTRANS_MULTI;
  L.multiOuts = (uint32_t)M;
  const size_t R = hoistedOperands(L, recs, what.c_str());
  size_t addends = 0, identities = 0;
  for (Instruction *i : recs) {
    if (i->ipLinPt.size() != M) throw std::runtime_error(what + ": the records of one launch form different numbers of sums");
    addends += i->ipLinAddend != 0;
    identities += !i->ipLinIdPt.empty();
  }
  if (identities && identities != addends) throw std::runtime_error(what + ": the identity step on some of the records with an addend only");
  auto outOf = [](const Instruction *i, size_t x) { return x == 0 ? i->OutputOperand : i->extraOutputs[x - 1]; };
  if (addends)
    for (Instruction *i : recs) L.d.push_back(i->ipLinAddend ? limb(i->ipLinAddend) : HM_NO_LIMB);
  if (identities)
    for (Instruction *i : recs) L.d1.push_back(i->ipLinAddend1 ? limb(i->ipLinAddend1) : HM_NO_LIMB);
  for (size_t m = 0; m < M; ++m) {
    for (Instruction *i : recs) {
      const size_t w = !i->ipLinIdPt.empty() ? 4 : i->ipLinAddend ? 3 : 2;
      L.out.push_back(limb(outOf(i, m * w))); L.out.push_back(limb(outOf(i, m * w + 1)));
      if (addends) L.out1.push_back(i->ipLinAddend ? limb(outOf(i, m * w + 2)) : HM_NO_LIMB);
      if (identities) {
        L.idPt.push_back(w == 4 ? limb(i->ipLinIdPt[m]) : HM_NO_LIMB);
        L.out2.push_back(w == 4 ? limb(outOf(i, m * w + 3)) : HM_NO_LIMB);
      }
    }
    for (size_t r = 0; r < R; ++r)
      for (Instruction *i : recs) L.c.push_back(limb(i->ipLinPt[m][r]));
  }
  // limb-polys touched: a workgroup serves a tile of sums (one sum: one tile), so the digits, the keys and the addend source are read once per tile
  // (every rotation gathers from the same ones); every sum's plaintexts once; two outputs per entry and sum and one per addend and sum
  const unsigned long long tiles = (M + HM_IP_LINTRANS_MULTI_TILE - 1) / HM_IP_LINTRANS_MULTI_TILE;
  // the identity step: on the entries that have it, the second source once per tile, every sum's identity plaintext and its second addend output
  L.bytes = ((unsigned long long)recs.size() * (tiles * (L.ipTerms + 2 * R * L.ipTerms) + M * R + 2 * M) + (unsigned long long)addends * (tiles + M) +
             (unsigned long long)identities * (tiles + 2 * M)) * LP;
}

// (6s) one sum of rotations of different ciphertexts: digits a [c][n][T], keys b [c][n][2][T], outputs out [n][2]; entries with addends: sources
// d [c][n], output out1 [n] (hm_ip_rotsum_desc)
void Arch::LaunchBuilder::ipRotsum(Launch &L, Recs recs) {
  L.kind = Launch::L_IP_ROTSUM;
  const size_t G = hoistedOperands(L, recs, "sum of rotations", /*digitsPerRotation=*/true);
  size_t addends = 0;
  for (Instruction *i : recs) addends += !i->ipSumAddend.empty();
  for (Instruction *i : recs) {
    L.out.push_back(limb(i->OutputOperand)); L.out.push_back(limb(i->extraOutputs[0]));
    if (addends) L.out1.push_back(i->ipSumAddend.empty() ? HM_NO_LIMB : limb(i->extraOutputs[1]));
  }
  for (size_t c = 0; c < G && addends; ++c)
    for (Instruction *i : recs) L.d.push_back(i->ipSumAddend.empty() ? HM_NO_LIMB : limb(i->ipSumAddend[c]));
  // with initial sums (all records or none): c = init [n][2], d1 = the initial addend sums [n] (hm_ip_rotsum_init_desc)
  size_t inits = 0, addInits = 0;
  for (Instruction *i : recs) { inits += !i->ipSumInit.empty(); addInits += i->ipSumAddendInit != 0; }
  if (inits && (inits != recs.size() || addInits != addends)) throw std::runtime_error("sum of rotations: initial sums on some of the records of one launch only");
  for (Instruction *i : recs) {
    if (!inits) break;
    L.c.push_back(limb(i->ipSumInit[0])); L.c.push_back(limb(i->ipSumInit[1]));
    if (addends) L.d1.push_back(i->ipSumAddendInit ? limb(i->ipSumAddendInit) : HM_NO_LIMB);
  }
  // limb-polys touched: every ciphertext's digits, keys and addend source once, two outputs per entry and one per entry with addends; the
  // initial sums once
  L.bytes = ((unsigned long long)recs.size() * (G * 3 * L.ipTerms + 2) + (unsigned long long)addends * (G + 1) + 2 * inits + addInits) * LP;
}

// transform x key on one GPU (7, 8, 7b): a = source, c = first-pass scratch of every (limb, digit); the digits' conversions as `probs`
void Arch::LaunchBuilder::nttIp(Launch &L, Recs recs) {
  L.kind = Launch::L_NTT_IP; L.statKey = "NTT";
  L.ipTerms = (uint32_t)recs[0]->ipX.size(); L.ipOuts = (uint32_t)recs[0]->ipY.size();
  unsigned long long lp = 0;
  for (Instruction *i : recs) {
    for (size_t j = 0; j < i->ipX.size(); ++j) {
      L.a.push_back(limb(i->ipSrc[j])); L.c.push_back(limb(i->ipX[j])); L.ipCoeff.push_back(i->ipCoeff[j]);
      lp += i->ipCoeff[j] ? 3 : 1;       // transformed digit: source read, hand-off written and read; own limb: read
    }
    for (size_t j = 0; j < i->ipConvIn.size(); ++j) {   // (8): the digit's conversion runs inside its first pass
      if (i->ipConvIn[j].empty()) continue;
      Launch::Prob &pr = findOrAddProb(L, limbs(i->ipConvIn[j]), i->ipConvMods[j], j < i->ipConvPacked.size() && i->ipConvPacked[j]);
      pr.out.push_back(limb(i->ipX[j]));      // the hand-off limb of (limb, digit)
      pr.outMods.push_back(i->mod_id);
      lp -= 1;                                      // the converted limb is neither written nor read: source = the conversion's inputs
    }
    keyProductRecord(L, i);
    L.ipInv.push_back(i->ipInvOut ? 1 : 0);
    lp += (unsigned long long)L.ipTerms * L.ipOuts + L.ipOuts;
  }
  for (auto &q : L.probs) lp += q.in.size();
  L.bytes = lp * LP;
}

void Arch::LaunchBuilder::ip(Launch &L, Recs recs) {
  L.kind = Launch::L_IP; L.statKey = "EWE";
  L.ipTerms = (uint32_t)recs[0]->ipX.size(); L.ipOuts = (uint32_t)recs[0]->ipY.size();
  for (Instruction *i : recs) {
    for (AddrType x : i->ipX) L.a.push_back(limb(x));
    keyProductRecord(L, i);
  }
  L.bytes = (unsigned long long)(L.ipTerms * (1 + L.ipOuts) + L.ipOuts) * LP * recs.size();
}

void Arch::LaunchBuilder::tensor(Launch &L, Recs recs) {
  L.kind = Launch::L_TENSOR; L.statKey = "EWE";
  for (Instruction *i : recs) {  // a = c00 (P), b = c10 (T), c = c01 (R), d = c11 (S)
    L.a.push_back(limb(i->operandList[0])); L.b.push_back(limb(i->operandList[3]));
    L.c.push_back(limb(i->operandList[2])); L.d.push_back(limb(i->operandList[1]));
    tensorOutputs(L, i);
  }
  L.bytes = 7 * LP * recs.size();
}

// the three sums of a tensor form: out, out1, out2 = d0, d1, d2 [n]
void Arch::LaunchBuilder::tensorOutputs(Launch &L, const Instruction *i) {
  L.out.push_back(limb(i->extraOutputs[0])); L.out1.push_back(limb(i->OutputOperand)); L.out2.push_back(limb(i->extraOutputs[1]));
  L.mods.push_back(i->mod_id);
}

// (5q) a, c = c0, c1 of the ciphertext [n]; out, out1, out2 = d0, d1, d2 [n]; k / addK = the scalars / the constants [n] (hm_tensor_square).  The
// part key keeps records that absorbed different things apart
void Arch::LaunchBuilder::tensorSquare(Launch &L, Recs recs) {
  L.kind = Launch::L_TENSOR_SQUARE; L.statKey = "EWE";
  for (Instruction *i : recs) {
    L.a.push_back(limb(i->fu.reads[0])); L.c.push_back(limb(i->fu.reads[1]));
    tensorOutputs(L, i);
    if (recs[0]->fu.hasScale) L.k.push_back(i->fu.scales[0]);
    if (recs[0]->fu.hasConst) L.addK.push_back(i->fu.constant);
  }
  L.bytes = 5 * LP * recs.size();   // two polynomials read, three written
}

// (5l) a = the input of every term [n][T]; out = the sum [n]; k = the scalars [n][T], addK = the constants [n] (hm_lincomb).
// (5c) the same with k / maK = the real / the monomial parts of the scalars [n][T] (hm_clincomb; the back-end derives X^(N/2)): a (5l) record has
// no second scalar list.  The part key keeps records of different term counts apart; a record without a constant (c1 beside a c0 that has one)
// adds 0, which changes no residue
void Arch::LaunchBuilder::lincomb(Launch &L, Recs recs) {
  L.kind = recs[0]->fu.form == FusedForm::CLincomb ? Launch::L_CLINCOMB : Launch::L_LINCOMB; L.statKey = "EWE";
  L.dotTerms = recs[0]->fu.terms;
  for (Instruction *i : recs) {
    for (AddrType x : i->fu.reads) L.a.push_back(limb(x));
    L.k.insert(L.k.end(), i->fu.scales.begin(), i->fu.scales.end());
    L.maK.insert(L.maK.end(), i->fu.scales2.begin(), i->fu.scales2.end());
    L.out.push_back(limb(i->OutputOperand));
    L.mods.push_back(i->mod_id);
  }
  if (std::any_of(recs.begin(), recs.end(), [](const Instruction *i) { return i->fu.hasConst; }))
    for (Instruction *i : recs) L.addK.push_back(i->fu.hasConst ? i->fu.constant : 0);
  L.bytes = (L.dotTerms + 1ull) * LP * recs.size();   // every input read once, the sum written once
}

// (5L) a = the input of every term [n][T]; out = the M sums [n][M]; k = the scalars [n][M][T], addK = the constants [n][M] (hm_lincomb_multi).  The
// part key keeps records of different term and sum counts apart; a record without constants (c1 beside a c0 that has them) adds 0.  The back-end
// reads the inputs once per tile of HM_LINCOMB_MULTI_TILE sums
void Arch::LaunchBuilder::lincombMulti(Launch &L, Recs recs) {
  L.kind = Launch::L_LINCOMB_MULTI; L.statKey = "EWE";
  L.dotTerms = recs[0]->fu.terms;
  L.multiOuts = (uint32_t)recs[0]->fu.rowScales.size();
  for (Instruction *i : recs) {
    for (AddrType x : i->fu.reads) L.a.push_back(limb(x));
    for (const std::vector<uint64_t> &row : i->fu.rowScales) L.k.insert(L.k.end(), row.begin(), row.end());
    L.out.push_back(limb(i->OutputOperand));
    for (AddrType o : i->extraOutputs) L.out.push_back(limb(o));
    L.mods.push_back(i->mod_id);
  }
  if (std::any_of(recs.begin(), recs.end(), [](const Instruction *i) { return i->fu.hasConst; }))
    for (Instruction *i : recs) L.addK.insert(L.addK.end(), i->fu.rowConsts.begin(), i->fu.rowConsts.end());
  const unsigned long long tiles = (L.multiOuts + HM_LINCOMB_MULTI_TILE - 1) / HM_LINCOMB_MULTI_TILE;
  L.bytes = (tiles * L.dotTerms + L.multiOuts) * LP * recs.size();   // every input read once per tile of sums, every sum written once
}

// (5m) a, b, c, d = c00, c10, c01, c11 [n]; x0, x1 = c0, c1 of every addend [n][A]; out, out1, out2 = d0, d1, d2 [n]; k = the scalars [n], maK = the
// addend scalars [n][A], addK = the constants [n] (hm_tensor_muladd).  The part key keeps records of different addend counts, and records that
// absorbed different things, apart
void Arch::LaunchBuilder::tensorMulAdd(Launch &L, Recs recs) {
  L.kind = Launch::L_TENSOR_MULADD; L.statKey = "EWE";
  L.maAddends = recs[0]->fu.addends;
  for (Instruction *i : recs) {
    const std::vector<AddrType> &r = i->fu.reads;
    L.a.push_back(limb(r[0])); L.b.push_back(limb(r[1])); L.c.push_back(limb(r[2])); L.d.push_back(limb(r[3]));
    for (uint32_t t = 0; t < L.maAddends; ++t) {
      L.x0.push_back(limb(r[4 + 2 * t])); L.x1.push_back(limb(r[5 + 2 * t]));
    }
    L.maK.insert(L.maK.end(), i->fu.scales2.begin(), i->fu.scales2.end());
    tensorOutputs(L, i);
    if (recs[0]->fu.hasScale) L.k.push_back(i->fu.scales[0]);
    if (recs[0]->fu.hasConst) L.addK.push_back(i->fu.constant);
  }
  L.bytes = (7ull + 2 * L.maAddends) * LP * recs.size();   // four operands and both components of every addend read once, three polynomials written
}

// (5r) a = the polynomial, c = its conjugate [n]; out = their sum, out1 = U (.) their difference [n] (hm_reim_split; the back-end derives U)
void Arch::LaunchBuilder::reim(Launch &L, Recs recs) {
  L.kind = Launch::L_REIM; L.statKey = "EWE";
  for (Instruction *i : recs) {
    L.a.push_back(limb(i->fu.reads[0])); L.c.push_back(limb(i->fu.reads[1]));
    L.out.push_back(limb(i->OutputOperand)); L.out1.push_back(limb(i->extraOutputs[0]));
    L.mods.push_back(i->mod_id);
  }
  L.bytes = 4 * LP * recs.size();   // two polynomials read, two written
}

// (5p) b = the plaintext, x0 / x1 = c0 / c1 of the ciphertext of every term [n][T]; d = the addend [n] (empty: no record has one); out / out1 = the
// sums of c0 / c1 [n] (hm_plincomb).  The part key keeps records of different term counts apart, and those with an addend from those without
void Arch::LaunchBuilder::plincomb(Launch &L, Recs recs) {
  L.kind = Launch::L_PLINCOMB; L.statKey = "EWE";
  L.dotTerms = recs[0]->fu.terms;
  const bool addend = recs[0]->fu.hasAddend;
  for (Instruction *i : recs) {
    const std::vector<AddrType> &r = i->fu.reads;
    for (uint32_t t = 0; t < L.dotTerms; ++t) {
      L.b.push_back(limb(r[3 * t])); L.x0.push_back(limb(r[3 * t + 1])); L.x1.push_back(limb(r[3 * t + 2]));
    }
    if (addend) L.d.push_back(limb(r[3 * L.dotTerms]));
    L.out.push_back(limb(i->OutputOperand)); L.out1.push_back(limb(i->extraOutputs[0]));
    L.mods.push_back(i->mod_id);
  }
  L.bytes = (3ull * L.dotTerms + 2 + (addend ? 1 : 0)) * LP * recs.size();   // plaintext and both components of every term read once, two sums written
}

// (5a) a, b, c, d = c00, c10, c01, c11 of every pair [n][T]; x0, x1 = c0, c1 of every addend [n][A]; out, out1, out2 = d0, d1, d2 [n]; k = the pair
// scalars [n][T], maK = the addend scalars [n][A], addK = the constants [n] (hm_tensor_dotadd).  The part key keeps records of different pair
// and addend counts apart; a record without scalars beside one that has them multiplies by 1, one without a constant adds 0: neither changes a
// residue.
// (5d) the same without addends, scalars and constant (hm_tensor_dot): a (5d) record carries none of them
void Arch::LaunchBuilder::tensorDotAdd(Launch &L, Recs recs) {
  L.kind = recs[0]->fu.form == FusedForm::TensorDot ? Launch::L_TENSOR_DOT : Launch::L_TENSOR_DOTADD; L.statKey = "EWE";
  L.dotTerms = recs[0]->fu.terms;
  L.maAddends = recs[0]->fu.addends;
  const bool scaled = std::any_of(recs.begin(), recs.end(), [](const Instruction *i) { return i->fu.hasScale; });
  const bool shifted = std::any_of(recs.begin(), recs.end(), [](const Instruction *i) { return i->fu.hasConst; });
  for (Instruction *i : recs) {
    const std::vector<AddrType> &r = i->fu.reads;
    for (size_t t = 0; t < L.dotTerms; ++t) {
      L.a.push_back(limb(r[4 * t])); L.b.push_back(limb(r[4 * t + 1])); L.c.push_back(limb(r[4 * t + 2])); L.d.push_back(limb(r[4 * t + 3]));
    }
    for (size_t a = 0; a < L.maAddends; ++a) {
      L.x0.push_back(limb(r[4 * L.dotTerms + 2 * a])); L.x1.push_back(limb(r[4 * L.dotTerms + 2 * a + 1]));
    }
    if (scaled) L.k.insert(L.k.end(), i->fu.scales.begin(), i->fu.scales.end());
    L.maK.insert(L.maK.end(), i->fu.scales2.begin(), i->fu.scales2.end());
    if (shifted) L.addK.push_back(i->fu.hasConst ? i->fu.constant : 0);
    tensorOutputs(L, i);
  }
  L.bytes = (4ull * L.dotTerms + 2 * L.maAddends + 3) * LP * recs.size();   // every operand and both components of every addend read once, three sums written
}

// fused forward transform (4, 4b, 9, 12)
void Arch::LaunchBuilder::nttSubScale(Launch &L, Recs recs) {
  L.kind = Launch::L_NTT_SUBSCALE; L.statKey = "NTT";
  bool anyAddend = false;   // the addend is per limb-poly (hrotate: key 0 adds the rotated c0, key 1 nothing)
  bool anyAddGalois = false;   // (12) ... and key 0's addend through the automorphism
  for (Instruction *i : recs) { anyAddend |= i->fAddend != 0; anyAddGalois |= i->fAddendGalois != 0; }
  for (Instruction *i : recs) {
    L.a.push_back(limb(i->operandList[0])); L.b.push_back(limb(i->fMinuend));
    if (recs[0]->fMinuendB) L.mulB.push_back(limb(i->fMinuendB));   // the part key keeps product and plain minuends apart
    if (anyAddend) L.c.push_back(i->fAddend ? limb(i->fAddend) : HM_NO_LIMB);
    if (anyAddGalois) L.addGalois.push_back(i->fAddendGalois);
    L.out.push_back(limb(i->OutputOperand)); L.mods.push_back(i->mod_id); L.k.push_back(i->constant);
    if (recs[0]->fMix) {  // the part key keeps merged and plain records apart
      L.d.push_back(limb(i->fMix)); L.mixK.push_back(i->fMixConst);
      if (anyAddend) L.addK.push_back(i->fAddendConst ? i->fAddendConst : 1);
    }
  }
  L.hasK = true;
  L.bytes = ((anyAddend ? 4 : 3) + (L.mulB.empty() ? 0 : 1)) * LP * recs.size();
  for (Instruction *i : recs) {   // (9): the conversion of this limb-poly runs inside its first pass
    if (i->fConvIn.empty()) continue;
    bool added;
    Launch::Prob &pr = findOrAddProb(L, limbs(i->fConvIn), i->fConvMods, i->inPacked, false, false, &added);
    if (added) L.bytes += LP * pr.in.size();
    pr.out.push_back(limb(i->OutputOperand));   // the hand-off lands in the output limb
    pr.outMods.push_back(i->mod_id);
    L.bytes -= LP;                                  // the converted limb-poly is neither written nor read
  }
}

// unfused mode: a pass-through transform materialises its copy
void Arch::LaunchBuilder::copy(Launch &L, Recs recs) {
  L.kind = Launch::L_EWE; L.opcode = EWE_COPY; L.statKey = "EWE";
  for (Instruction *i : recs) { L.a.push_back(limb(i->operandList[0])); L.out.push_back(limb(i->OutputOperand)); L.mods.push_back(i->mod_id); }
  L.bytes = 2 * LP * recs.size();
}

void Arch::LaunchBuilder::transform(Launch &L, Recs recs) {
  Instruction *f = recs[0];
  L.kind = f->ops == NTT ? Launch::L_NTT : Launch::L_INTT; L.statKey = "NTT";
  L.secondOnly = f->secondOnly;
  bool anyInGalois = false;
  for (Instruction *i : recs) anyInGalois |= i->inGalois != 0;
  for (Instruction *i : recs) {
    if (anyInGalois) L.inGalois.push_back(i->inGalois);
    L.a.push_back(limb(i->operandList[0])); L.out.push_back(limb(i->OutputOperand)); L.mods.push_back(i->mod_id);
    L.k.push_back(i->hasConstant ? i->constant : 1);
    L.hasK |= i->hasConstant;
    if (f->ops == INTT) L.outPacked.push_back(i->packedOut ? 1 : 0);
    if (f->inMulB) L.mulB.push_back(limb(i->inMulB));   // (the part key keeps product and plain inputs apart)
    if (f->liftSrcMod != kNoLift) L.liftMods.push_back(i->liftSrcMod);   // (... and lifted and plain inputs)
  }
  L.bytes = (L.mulB.empty() ? 2 : 3) * LP * recs.size();
  if (!L.liftMods.empty()) {   // many records read one source: every distinct source once, every output once
    std::vector<uint32_t> src = L.a;
    std::sort(src.begin(), src.end());
    L.bytes = LP * ((size_t)(std::unique(src.begin(), src.end()) - src.begin()) + recs.size());
  }
}

void Arch::LaunchBuilder::automorphism(Launch &L, Recs recs) {
  L.kind = Launch::L_AUTO; L.statKey = "AUTO"; L.galois = recs[0]->galois;
  for (Instruction *i : recs) { L.a.push_back(limb(i->operandList[0])); L.out.push_back(limb(i->OutputOperand)); }
  L.bytes = 2 * LP * recs.size();
}

void Arch::LaunchBuilder::ewe(Launch &L, Recs group) {
  L.kind = Launch::L_EWE; L.opcode = group[0]->opcode; L.statKey = "EWE";
  const int m = eweOperandMask(group[0]->opcode);
  int nops = 1;
  for (int b = 0; b < 4; ++b) nops += (m >> b) & 1;
  // entries of one modulus side by side: records that share an operand (pmult: c0 x pt and c1 x pt of a limb) then sit 128 workgroups apart
  // in dispatch order, on the same XCD, and the second reader finds the shared limb-poly in L2 instead of fetching it again
  std::vector<Instruction *> recs = group;
  std::stable_sort(recs.begin(), recs.end(), [](const Instruction *x, const Instruction *y) { return x->mod_id < y->mod_id; });
  for (Instruction *i : recs) {
    auto get = [&](int b) { return (m & (1 << b)) ? limb(i->operandList[b]) : 0u; };
    L.a.push_back(get(0)); L.b.push_back(get(1)); L.c.push_back(get(2)); L.d.push_back(get(3));
    L.out.push_back(limb(i->OutputOperand)); L.mods.push_back(i->mod_id);
    L.k.push_back(i->hasConstant ? i->constant : 0);
    L.hasK |= i->hasConstant;
  }
  L.bytes = (unsigned long long)nops * LP * recs.size();
}

// one conversion per distinct (input limbs, epilogue form, input form)
void Arch::LaunchBuilder::bconv(Launch &L, Recs recs) {
  L.kind = Launch::L_BCONV; L.statKey = "BCONV";
  for (Instruction *i : recs) {
    std::vector<AddrType> convIn;
    for (size_t x = 0; x + 1 < i->operandList.size(); ++x) convIn.push_back(i->operandList[x]);
    Launch::Prob &pr = findOrAddProb(L, limbs(convIn), i->inMods, i->inPacked, i->fusedEpi, i->fAdd != 0);
    pr.out.push_back(limb(i->OutputOperand));
    pr.outMods.push_back(i->mod_id);
    if (i->fusedEpi) {   // (10): out = (fSubFrom - conv) * k [+ fAdd]
      pr.epA.push_back(limb(i->fSubFrom)); pr.epK.push_back(i->constant);
      if (i->fAdd) pr.epB.push_back(limb(i->fAdd));
      L.bytes += LP * (i->fAdd ? 2 : 1);
    }
  }
  if (A.world_ > 1 && A.batch_ > 1 && !A.shardGather) {  // sharded batch: the ops of the batch share the exchanges around the conversion
    const uint32_t per = (uint32_t)A.limbIndex.size();
    const size_t p0 = L.probs.size();
    for (uint32_t c = 1; c < A.batch_; ++c)
      for (size_t i = 0; i < p0; ++i) {
        Launch::Prob q = L.probs[i];
        for (uint32_t &x : q.in) x += c * per;
        for (uint32_t &x : q.out) x += c * per;
        L.probs.push_back(q);
      }
    L.refInstructions *= A.batch_;
  }
  for (auto &q : L.probs) L.bytes += LP * (q.in.size() + q.out.size());
}

// all-to-all plan: limb-sharded -> coefficient slices -> convert every output on this rank's slice -> limb-sharded
void Arch::LaunchBuilder::wrapShardedConversion(LaunchPtr L, Recs recs, Launches &front, Launches &back) {
  LaunchPtr XI = std::make_unique<Launch>(), XO = std::make_unique<Launch>();
  XI->kind = Launch::L_EXCH_IN; XO->kind = Launch::L_EXCH_OUT; XI->statKey = XO->statKey = "XCHG";
  XI->name = L->name + ":limbs->slices"; XO->name = L->name + ":slices->limbs";
  for (auto &q : L->probs) {
    for (size_t x = 0; x < q.in.size(); ++x)
      if (std::find(XI->exLimbs.begin(), XI->exLimbs.end(), q.in[x]) == XI->exLimbs.end()) { XI->exLimbs.push_back(q.in[x]); XI->exOwners.push_back(A.owner(q.inMods[x])); }
    for (size_t x = 0; x < q.out.size(); ++x) { XO->exLimbs.push_back(q.out[x]); XO->exOwners.push_back(A.owner(q.outMods[x])); }
  }
  std::vector<uint32_t> inRows(XI->exLimbs.size()), outRows(XO->exLimbs.size());
  hm_slice_rows(XI->exOwners.data(), (uint32_t)inRows.size(), A.world_, inRows.data());
  hm_slice_rows(XO->exOwners.data(), (uint32_t)outRows.size(), A.world_, outRows.data());
  size_t o = 0;
  for (auto &q : L->probs) {
    for (uint32_t &x : q.in) x = inRows[std::find(XI->exLimbs.begin(), XI->exLimbs.end(), x) - XI->exLimbs.begin()];
    for (uint32_t &x : q.out) x = outRows[o++];
  }
  L->logLen = XI->logLen = XO->logLen = A.logN - (uint32_t)__builtin_ctz(A.world_);
  XI->bytes = LP * XI->exLimbs.size() / A.world_;
  XO->bytes = LP * XO->exLimbs.size() / A.world_;
  L->bytes /= A.world_;
  if (A.pipelineDigits) {
    XI->waitSlots = L->waitSlots;   // (its inputs come from the compute stream; marks matter only if an exchange produced them)
    XI->recordSlot = nextSlot++;
    L->waitSlots = {XI->recordSlot};
    XO->recordSlot = nextSlot++;
    for (Instruction *i : recs) slotOfAddr[i->OutputOperand] = XO->recordSlot;
  }
  L->xin = XI.get(); L->xout = XO.get();
  A.algBytes += L->bytes;
  (A.pipelineDigits ? front : back).push_back(std::move(XI));
  back.push_back(std::move(L));
  back.push_back(std::move(XO));
}

// one launch for the records of a group (all of one part key)
void Arch::LaunchBuilder::emitCompute(const Group &group, Launches &front, Launches &back) {
  const std::vector<Instruction *> recs = flatten(group);
  Instruction *f = recs[0];
  LaunchPtr L = std::make_unique<Launch>();
  xGaloisSet = false;
  if (A.pipelineDigits)
    for (const Part *g : group) for (int sl : slotsOf(g)) addUnique(L->waitSlots, sl);
  for (const Part *g : group) L->name += (L->name.empty() ? "" : "+") + g->name;
  for (Instruction *i : recs) L->refInstructions += i->refInstructions * (i->ops == BCONV_STEP2 ? bconvPorts : 1ull) + i->refExtra;
  if (f->ops == IP && !f->ipSumX.empty()) ipRotsum(*L, recs);
  else if (f->ops == IP && !f->ipLinPt.empty()) ipLintrans(*L, recs);
  else if (f->ops == IP && !f->ipHoistG.empty()) ipHoisted(*L, recs);
  else if (f->ops == IP && transformsInside(*f)) nttIp(*L, recs);
  else if (isKeyProduct(*f)) ip(*L, recs);
  else if (f->fu.form != FusedForm::None)
    switch (f->fu.form) {
      case FusedForm::TensorDot: case FusedForm::DotAdd: tensorDotAdd(*L, recs); break;
      case FusedForm::Square: tensorSquare(*L, recs); break;
      case FusedForm::Lincomb: case FusedForm::CLincomb: lincomb(*L, recs); break;
      case FusedForm::LincombMulti: lincombMulti(*L, recs); break;
      case FusedForm::MulAdd: tensorMulAdd(*L, recs); break;
      case FusedForm::ReIm: reim(*L, recs); break;
      case FusedForm::PLincomb: plincomb(*L, recs); break;
      case FusedForm::None: break;
    }
  else if (f->fusedTensor) tensor(*L, recs);
  else if (f->fusedSubScale) nttSubScale(*L, recs);
  else if (f->ops == NTT && f->passthrough) copy(*L, recs);
  else if (f->ops == NTT || f->ops == INTT) transform(*L, recs);
  else if (f->ops == AUTO) automorphism(*L, recs);
  else if (f->ops == MULT) ewe(*L, recs);
  else if (f->ops == BCONV_STEP2) {
    bconv(*L, recs);
    if (A.world_ > 1 && !A.shardGather) return wrapShardedConversion(std::move(L), recs, front, back);
  } else throw std::runtime_error("no unit executes op " + f->GetOpName());
  A.algBytes += L->bytes;
  back.push_back(std::move(L));
}

// sharded ModUp with the fused kernels (round 4).  Per digit j: limbs -> COLUMN slices of the digit's limbs (all-to-all), conversion +
// first pass on this rank's columns for EVERY output limb (hm_bconv_col), column slices -> limbs of the first-pass hand-off
// (all-to-all back); then ONE transform x key launch over this rank's extended limbs (second pass + MAC with both keys).
// Every rank issues every exchange (the lists come from the global graph), also a rank that owns no extended limb.
void Arch::LaunchBuilder::shardedTransformTimesKey(const Group &group) {
  const std::vector<Instruction *> recs = flatten(group);
  Launch digs;   // per digit (probs): in = the conversion's inputs, out = the hand-off limbs of every extended limb
  for (Instruction *i : recs)
    for (size_t j = 0; j < i->ipConvIn.size(); ++j) {
      if (i->ipConvIn[j].empty()) continue;
      Launch::Prob &dg = findOrAddProb(digs, limbs(i->ipConvIn[j]), i->ipConvMods[j], false);
      dg.out.push_back(limb(i->ipX[j]));
      dg.outMods.push_back(i->mod_id);
    }
  const uint32_t per = (uint32_t)A.limbIndex.size();
  Launches front, back;
  std::vector<int> outSlots;
  const uint32_t nTiles = cap(A.logN, "cap_col_slices") / A.world_;   // column tiles of a limb-poly per rank
  for (size_t dj = 0; dj < digs.probs.size(); ++dj) {
    const Launch::Prob &dg = digs.probs[dj];
    LaunchPtr XI = std::make_unique<Launch>(), BC = std::make_unique<Launch>(), XO = std::make_unique<Launch>();
    XI->kind = Launch::L_EXCH_IN_COL; BC->kind = Launch::L_BCONV_COL; XO->kind = Launch::L_EXCH_OUT_COL;
    XI->statKey = XO->statKey = "XCHG"; BC->statKey = "BCONV";
    BC->name = "ModUp_BCONV_COL_(" + std::to_string(dj) + ")";
    XI->name = BC->name + ":limbs->columns"; XO->name = BC->name + ":columns->limbs";
    for (uint32_t c = 0; c < A.batch_; ++c) {   // the ops of a batch share the exchanges
      for (size_t x = 0; x < dg.in.size(); ++x) { XI->exLimbs.push_back(dg.in[x] + c * per); XI->exOwners.push_back(A.owner(dg.inMods[x])); }
      for (size_t x = 0; x < dg.out.size(); ++x) { XO->exLimbs.push_back(dg.out[x] + c * per); XO->exOwners.push_back(A.owner(dg.outMods[x])); }
    }
    std::vector<uint32_t> inRows(XI->exLimbs.size()), outRows(XO->exLimbs.size());
    hm_slice_rows(XI->exOwners.data(), (uint32_t)inRows.size(), A.world_, inRows.data());
    hm_slice_rows(XO->exOwners.data(), (uint32_t)outRows.size(), A.world_, outRows.data());
    for (uint32_t c = 0; c < A.batch_; ++c) {
      Launch::Prob q{{}, dg.inMods, {}, dg.outMods};
      for (size_t x = 0; x < dg.in.size(); ++x) q.in.push_back(inRows[c * dg.in.size() + x]);
      for (size_t x = 0; x < dg.out.size(); ++x) q.out.push_back(outRows[c * dg.out.size() + x]);
      BC->probs.push_back(q);
    }
    BC->galois = A.rank_ * nTiles;    // first column tile of this rank's slice
    BC->logLen = nTiles;            // ... and how many
    BC->refInstructions = 0;        // (accounted on the transform x key launch, as in the one-GPU plan)
    XI->bytes = LP * XI->exLimbs.size() / A.world_;
    XO->bytes = LP * XO->exLimbs.size() / A.world_;
    BC->bytes = (XI->bytes + XO->bytes);
    if (A.pipelineDigits) {
      XI->recordSlot = nextSlot++;
      BC->waitSlots = {XI->recordSlot};
      XO->recordSlot = nextSlot++;
    }
    outSlots.push_back(XO->recordSlot);
    BC->xin = XI.get(); BC->xout = XO.get();
    A.algBytes += BC->bytes;
    (A.pipelineDigits ? front : back).push_back(std::move(XI));
    back.push_back(std::move(BC));
    back.push_back(std::move(XO));
  }
  // this rank's extended limbs: the one-GPU launch's operands, but a converted digit arrives as its first-pass hand-off (ipCoeff 2) and no
  // conversion runs inside
  LaunchPtr L = std::make_unique<Launch>();
  xGaloisSet = false;
  L->kind = Launch::L_NTT_IP; L->statKey = "NTT";
  L->ipTerms = (uint32_t)recs[0]->ipX.size(); L->ipOuts = (uint32_t)recs[0]->ipY.size();
  unsigned long long lp = 0;
  for (const Part *g : group) {
    bool any = false;
    for (Instruction *i : g->ins) {
      if (!mine(i)) continue;
      L->refInstructions += i->refInstructions;
      any = true;
      for (size_t j = 0; j < i->ipX.size(); ++j) {
        const bool conv = j < i->ipConvIn.size() && !i->ipConvIn[j].empty();
        L->a.push_back(limb(i->ipSrc[j])); L->c.push_back(limb(i->ipX[j]));
        L->ipCoeff.push_back(conv ? 2 : i->ipCoeff[j]);
        lp += 1;
      }
      keyProductRecord(*L, i);
      lp += (unsigned long long)L->ipTerms * L->ipOuts + L->ipOuts;
    }
    if (any) L->name += (L->name.empty() ? "" : "+") + g->name;
  }
  L->bytes = lp * LP;
  if (A.pipelineDigits) for (int sl : outSlots) L->waitSlots.push_back(sl);
  append(front);
  append(back);
  // (a rank without extended limbs still waits for nothing: its exchanges are complete on their own stream)
  if (!L->mods.empty()) { A.algBytes += L->bytes; A.launches.push_back(std::move(L)); }
}

// operands written on another rank (the rescale's r = INTT(x_last); with the gather plan also the conversions' inputs): replicate them
// first — every rank derives the same list from the global graph, so the collective is entered by all
void Arch::LaunchBuilder::replicateForeignOperands(const Group &group) {
  std::vector<AddrType> need;
  for (Instruction *i : flatten(group))
    for (AddrType a : loads(*i)) {
      auto oo = ownerOfAddr.find(a);
      if (oo != ownerOfAddr.end() && oo->second != A.owner(i->mod_id) && std::find(need.begin(), need.end(), a) == need.end()) need.push_back(a);
    }
  if (need.empty()) return;
  LaunchPtr R = std::make_unique<Launch>();
  R->kind = Launch::L_REPLICATE; R->statKey = "XCHG"; R->name = "replicate";
  for (AddrType a : need) { R->exLimbs.push_back(limb(a)); R->exOwners.push_back(ownerOfAddr[a]); }
  R->bytes = LP * need.size();
  if (A.pipelineDigits) {
    for (AddrType a : need) { auto it = slotOfAddr.find(a); if (it != slotOfAddr.end()) addUnique(R->waitSlots, it->second); }
    R->recordSlot = nextSlot++;
    for (AddrType a : need) slotOfAddr[a] = R->recordSlot;
  }
  A.launches.push_back(std::move(R));
}

std::set<int> Arch::LaunchBuilder::slotsOf(const Part *g) const {
  std::set<int> ss;
  for (Instruction *i : g->ins)
    for (AddrType a : loads(*i)) { auto it = slotOfAddr.find(a); if (it != slotOfAddr.end()) ss.insert(it->second); }
  return ss;
}

// pipelined sharded plan: parts that depend on different exchanges (digit j's transforms read what exchange XO_j delivered)
// become launches of their own, each waiting for its own mark; the conversions are split by input basis (= by digit; the two
// keys of a ModDown share theirs and stay together).  Exchange-in launches of all digits are issued first.
std::vector<Group> Arch::LaunchBuilder::splitByExchangeMark(const Group &group) const {
  std::vector<Group> subgroups;
  std::vector<std::set<int>> sigs;
  std::vector<std::vector<uint32_t>> bases;
  const bool isConv = group[0]->ins[0]->ops == BCONV_STEP2;
  for (const Part *g : group) {
    const std::set<int> sg = slotsOf(g);
    const std::vector<uint32_t> bs = isConv ? g->ins[0]->inMods : std::vector<uint32_t>();
    size_t k = 0;
    for (; k < subgroups.size(); ++k) if (sigs[k] == sg && bases[k] == bs) break;
    if (k == subgroups.size()) { subgroups.emplace_back(); sigs.push_back(sg); bases.push_back(bs); }
    subgroups[k].push_back(g);
  }
  return subgroups;
}

// the parts of one depth and key -> launches
void Arch::LaunchBuilder::emitGroup(Group group) {
  Instruction *f = group[0]->ins[0];
  if (A.world_ > 1 && f->ops == IP && !A.shardGather) {
    bool fusedConversion = false;
    for (Instruction *i : flatten(group))
      for (auto &cin : i->ipConvIn) fusedConversion |= !cin.empty();
    if (fusedConversion) return shardedTransformTimesKey(group);
  }
  std::vector<Part> mineParts;
  if (A.world_ > 1 && (f->ops != BCONV_STEP2 || A.shardGather)) {
    replicateForeignOperands(group);
    for (const Part *g : group) {   // keep the instructions whose modulus this rank owns
      Part m{g->name, g->key, {}, g->depth};
      for (Instruction *i : g->ins)
        if (mine(i)) m.ins.push_back(i);
      if (!m.ins.empty()) mineParts.push_back(m);
    }
    group.clear();
    for (const Part &m : mineParts) group.push_back(&m);
    if (group.empty()) return;
  }
  Launches front, back;
  for (const Group &sub : A.pipelineDigits ? splitByExchangeMark(group) : std::vector<Group>{group}) emitCompute(sub, front, back);
  append(front);
  append(back);
}

void Arch::buildLaunches() {
  std::vector<Stage> st = stages;
  if (fuse) fusePasses(st);
  // 1. split every stage into parts one C-ABI call can express
  std::vector<Part> parts;
  for (const Stage &s : st) {
    const size_t first = parts.size();
    for (Instruction *i : s.ins) {
      const int key = partKey(*i);
      size_t p = first;
      while (p < parts.size() && parts[p].key != key) ++p;
      if (p == parts.size()) parts.push_back(Part{s.name, key, {}, 0});
      parts[p].ins.push_back(i);
    }
  }
  // 2. dependency depth
  assignDepths(parts, fuse);
  // (only the plan that holds a square's tensor record which pass (5q) did not take: fuse_square = 0.  Every other plan keeps the plain
  // level-by-level order it is pinned to, launch by launch: tests/golden/plan_fingerprints.json)
  const bool plainSquare = std::any_of(parts.begin(), parts.end(), [](const Part &p) { return p.ins[0]->mark == FusedForm::Square && p.ins[0]->fusedTensor && p.ins[0]->fu.form == FusedForm::None; });
  // (... and the plan that holds a marked product's tensor record which pass (5m) did not take: fuse_muladd = 0)
  const bool plainMuladd = std::any_of(parts.begin(), parts.end(), [](const Part &p) { return p.ins[0]->mark == FusedForm::MulAdd && p.ins[0]->fusedTensor && p.ins[0]->fu.form == FusedForm::None; });
  if (fuse && world_ == 1 && (plainSquare || plainMuladd)) joinEarlierGroups(parts);
  LaunchBuilder b(*this);
  // multi-GPU: who holds each limb-poly.  Inputs: by the modulus they were filled for; everything else: by the modulus of the
  // instruction that writes it.
  if (world_ > 1) {
    for (const InputFill &f : fills)
      for (size_t i = 0; i < f.addrs.size(); ++i) b.ownerOfAddr[f.addrs[i]] = owner(f.mods[i]);
    for (const Part &p : parts)
      for (Instruction *i : p.ins)
        for (const Write &o : recordWrites(*i)) b.ownerOfAddr[o.addr] = owner(i->mod_id);
  }
  // 3. coalesce and emit, level by level: the parts of equal depth and key, in the order of the first of them
  int maxDepth = 0;
  for (const Part &p : parts) maxDepth = std::max(maxDepth, p.depth);
  for (int d = 0; d <= maxDepth; ++d) {
    std::vector<int> keysDone;
    for (size_t pi = 0; pi < parts.size(); ++pi) {
      if (parts[pi].depth != d || std::find(keysDone.begin(), keysDone.end(), parts[pi].key) != keysDone.end()) continue;
      keysDone.push_back(parts[pi].key);
      Group group;
      for (size_t pj = pi; pj < parts.size(); ++pj)
        if (parts[pj].depth == d && parts[pj].key == parts[pi].key) group.push_back(&parts[pj]);
      b.emitGroup(group);
    }
  }
}

// batch > 1: every launch carries the limb-polys of `batch` independent ops.  Op c lives in its own copy of the
// buffer plan (limb index + c * limbs-per-op) with its own inputs (fill seed + c * kBatchSeedStride); buffers
// marked shared (the evaluation key: all ops of a batch are under the same key) exist once.  Larger launches
// amortise the per-launch latency and pair up same-modulus limb-polys across ops (one twiddle fetch per pair).
static const uint64_t kBatchSeedStride = 100000;
void Arch::replicateForBatch() {
  const uint32_t per = (uint32_t)limbIndex.size();
  std::set<uint32_t> sharedLimbs;
  for (const InputFill &f : fills)
    if (f.shared)
      for (AddrType a : f.addrs) sharedLimbs.insert(limbOf(a));
  auto rep = [&](std::vector<uint32_t> &v, bool isLimb) {
    const size_t n0 = v.size();
    for (uint32_t c = 1; c < batch_; ++c)
      for (size_t i = 0; i < n0; ++i) v.push_back(isLimb && v[i] != HM_NO_LIMB && !sharedLimbs.count(v[i]) ? v[i] + c * per : v[i]);
  };
  for (auto &l : launches) {
    if (world_ > 1 && !shardGather && (l->kind == Launch::L_BCONV || l->kind == Launch::L_EXCH_IN || l->kind == Launch::L_EXCH_OUT)) continue;  // built batched
    if (l->kind == Launch::L_BCONV_COL || l->kind == Launch::L_EXCH_IN_COL || l->kind == Launch::L_EXCH_OUT_COL) continue;           // built batched
    if (l->kind == Launch::L_REPLICATE) {
      const size_t n0 = l->exLimbs.size();
      for (uint32_t c = 1; c < batch_; ++c)
        for (size_t i = 0; i < n0; ++i) { l->exLimbs.push_back(l->exLimbs[i] + c * per); l->exOwners.push_back(l->exOwners[i]); }
      l->bytes *= batch_;
      continue;
    }
    if (l->kind == Launch::L_IP_HOISTED || l->kind == Launch::L_IP_LINTRANS || l->kind == Launch::L_IP_ROTSUM || l->kind == Launch::L_IP_LINTRANS_MULTI) {
      // entry-major as the inner product below (the ops of a batch share the keys), inside every rotation's block of keys and outputs
      const size_t n0 = l->mods.size();
      auto inter = [&](std::vector<uint32_t> &v, size_t blocks, size_t width, bool isLimb) {
        std::vector<uint32_t> o;
        for (size_t r = 0; r < blocks; ++r)
          for (size_t e = 0; e < n0; ++e)
            for (uint32_t c = 0; c < batch_; ++c)
              for (size_t w = 0; w < width; ++w) {
                const uint32_t x = v[(r * n0 + e) * width + w];
                o.push_back(isLimb && c && x != HM_NO_LIMB && !sharedLimbs.count(x) ? x + c * per : x);
              }
        v.swap(o);
      };
      const size_t R = l->hoistG.size();
      inter(l->a, l->kind == Launch::L_IP_ROTSUM ? R : 1, l->ipTerms, true); inter(l->b, R, 2 * (size_t)l->ipTerms, true); inter(l->mods, 1, 1, false);
      if (l->kind == Launch::L_IP_HOISTED) inter(l->out, R, 2, true);
      else if (l->kind == Launch::L_IP_ROTSUM) {   // every ciphertext its own digits and addend source
        inter(l->out, 1, 2, true);
        if (!l->d.empty()) { inter(l->d, R, 1, true); inter(l->out1, 1, 1, true); }
        if (!l->c.empty()) inter(l->c, 1, 2, true);   // every op its own initial sums
        if (!l->d1.empty()) inter(l->d1, 1, 1, true);
      } else {   // the weighted sums (one: L_IP_LINTRANS): every sum its own plaintexts and outputs
        const size_t M = l->multiOuts;
        inter(l->out, M, 2, true); inter(l->c, M * R, 1, true);
        if (!l->d.empty()) { inter(l->d, 1, 1, true); inter(l->out1, M, 1, true); }
        if (!l->d1.empty()) { inter(l->d1, 1, 1, true); inter(l->idPt, M, 1, true); inter(l->out2, M, 1, true); }   // every op its own identity plaintexts and outputs
      }
      l->refInstructions *= batch_;
      l->bytes *= batch_;
      continue;
    }
    if (l->kind == Launch::L_IP || l->kind == Launch::L_NTT_IP) {
      // entry e: ipTerms x limbs, ipTerms * ipOuts y limbs, ipOuts outputs.  Entry-major order (entry e of every op
      // side by side): the ops share the key limbs, so the second and later readers of a key chunk find it in L2
      auto inter = [&](std::vector<uint32_t> &v, size_t width, bool isLimb) {
        const size_t n0 = v.size() / width;
        std::vector<uint32_t> o;
        for (size_t e = 0; e < n0; ++e)
          for (uint32_t c = 0; c < batch_; ++c)
            for (size_t w = 0; w < width; ++w) {
              const uint32_t x = v[e * width + w];
              o.push_back(isLimb && c && !sharedLimbs.count(x) ? x + c * per : x);
            }
        v.swap(o);
      };
      inter(l->a, l->ipTerms, true); inter(l->b, (size_t)l->ipTerms * l->ipOuts, true); inter(l->out, l->ipOuts, true); inter(l->mods, 1, false);
      if (l->kind == Launch::L_NTT_IP) {
        const size_t p0 = l->probs.size();
        for (uint32_t c = 1; c < batch_; ++c)
          for (size_t i = 0; i < p0; ++i) {
            Launch::Prob q = l->probs[i];
            for (uint32_t &x : q.in) x += c * per;
            for (uint32_t &x : q.out) x += c * per;
            for (uint32_t &x : q.epA) x += c * per;
            for (uint32_t &x : q.epB) x += c * per;
            l->probs.push_back(q);
          }
        inter(l->c, l->ipTerms, true);
        std::vector<uint32_t> f(l->ipCoeff.begin(), l->ipCoeff.end());
        inter(f, l->ipTerms, false);
        l->ipCoeff.assign(f.begin(), f.end());
        std::vector<uint32_t> fi(l->ipInv.begin(), l->ipInv.end());
        inter(fi, 1, false);
        l->ipInv.assign(fi.begin(), fi.end());
      }
    } else {
      {
        const size_t n0 = l->outPacked.size();
        for (uint32_t c = 1; c < batch_; ++c)
          for (size_t i = 0; i < n0; ++i) l->outPacked.push_back(l->outPacked[i]);
      }
      rep(l->a, true); rep(l->b, true); rep(l->c, true); rep(l->d, true);
      rep(l->out, true); rep(l->out1, true); rep(l->out2, true); rep(l->mods, false);
      rep(l->inGalois, false); rep(l->addGalois, false); rep(l->mulB, true); rep(l->liftMods, false);
      rep(l->x0, true); rep(l->x1, true);
      for (std::vector<uint64_t> *kv : {&l->k, &l->mixK, &l->addK, &l->maK}) {
        const size_t k0 = kv->size();
        for (uint32_t c = 1; c < batch_; ++c)
          for (size_t i = 0; i < k0; ++i) kv->push_back((*kv)[i]);
      }
      const size_t p0 = l->probs.size();
      for (uint32_t c = 1; c < batch_; ++c)
        for (size_t i = 0; i < p0; ++i) {
          Launch::Prob q = l->probs[i];
          for (uint32_t &x : q.in) x += c * per;
          for (uint32_t &x : q.out) x += c * per;
          for (uint32_t &x : q.epA) x += c * per;
          for (uint32_t &x : q.epB) x += c * per;
          l->probs.push_back(q);
        }
    }
    l->refInstructions *= batch_;
    l->bytes *= batch_;
  }
  algBytes *= batch_;
}

void Arch::prepare() {
  if (prepared) return;
  prepared = true;
  buildLaunches();
  if (batch_ > 1) {
    replicateForBatch();
    stat->setStat("Batch", batch_);
  }
  stat->setStat("Launches", launches.size());
  stat->setStat("LimbPolys_resident", limbIndex.size());
  stat->setStat("HBM_stage_bytes", algBytes);
  if (backendKind != BACKEND_HIP) return;
  const size_t bytes = (size_t)limbIndex.size() * batch_ * n * 8;
  void *p = nullptr;
  if (hm_malloc(ctx, bytes, &p) != HM_OK) throw std::runtime_error(std::string("hm_malloc: ") + hm_last_error(ctx));
  pool = static_cast<uint64_t *>(p);
  if (world_ > 1) {
    if (!commReady) throw std::runtime_error("world > 1 but no transport was set (commInitRccl / commInitExternal)");
    if (pipelineDigits && hm_exchange_stream(ctx, 1) != HM_OK) throw std::runtime_error(std::string("hm_exchange_stream: ") + hm_last_error(ctx));
    for (auto &bc : launches) {
      if (bc->kind != Launch::L_BCONV_COL || !bc->xin) continue;
      Launch *xi = bc->xin, *xo = bc->xout;
      void *si = nullptr, *so = nullptr;   // limb-poly layout: a row per limb-poly, this rank's columns valid
      if (hm_malloc(ctx, (size_t)xi->exLimbs.size() * n * 8, &si) != HM_OK || hm_malloc(ctx, (size_t)xo->exLimbs.size() * n * 8, &so) != HM_OK)
        throw std::runtime_error(std::string("hm_malloc (column slices): ") + hm_last_error(ctx));
      sliceBuffers.push_back(si); sliceBuffers.push_back(so);
      xi->slicesIn = bc->slicesIn = static_cast<uint64_t *>(si);
      bc->slicesOut = xo->slicesOut = static_cast<uint64_t *>(so);
    }
    for (auto &bc : launches) {
      if (bc->kind != Launch::L_BCONV || !bc->xin) continue;
      Launch *xi = bc->xin, *xo = bc->xout;
      void *si = nullptr, *so = nullptr;
      if (hm_malloc(ctx, (size_t)xi->exLimbs.size() * (n / world_) * 8, &si) != HM_OK || hm_malloc(ctx, (size_t)xo->exLimbs.size() * (n / world_) * 8, &so) != HM_OK)
        throw std::runtime_error(std::string("hm_malloc (slices): ") + hm_last_error(ctx));
      sliceBuffers.push_back(si); sliceBuffers.push_back(so);
      xi->slicesIn = bc->slicesIn = static_cast<uint64_t *>(si);
      bc->slicesOut = xo->slicesOut = static_cast<uint64_t *>(so);
    }
  }
  std::set<AddrType> bound;
  for (Binding &b : bindings) {
    if (!b.src->prepared) throw std::runtime_error("bindInput: prepare the producer first");
    for (size_t i = 0; i < b.dst.size(); ++i)
      for (uint32_t c = 0; c < batch_; ++c) {
        b.dstLimbs.push_back(limbOf(b.dst[i]) + c * (uint32_t)limbIndex.size());
        b.srcLimbs.push_back(b.src->limbOf(b.srcAddrs[i]) + c * (uint32_t)b.src->limbIndex.size());
        b.mods.push_back(0);
      }
    bound.insert(b.dst.begin(), b.dst.end());
  }
  for (const InputFill &f : fills)
    for (uint32_t c = 0; c < (f.shared ? 1u : batch_); ++c) {
      if (!f.addrs.empty() && bound.count(f.addrs[0])) continue;  // this input comes from another op
      std::vector<uint32_t> limbs;
      for (AddrType a : f.addrs) limbs.push_back(limbOf(a) + c * (uint32_t)limbIndex.size());
      if (hm_fill_uniform(ctx, pool, limbs.data(), f.mods.data(), (uint32_t)limbs.size(), f.seed + c * kBatchSeedStride) != HM_OK)
        throw std::runtime_error(std::string("hm_fill_uniform: ") + hm_last_error(ctx));
    }
  hm_sync(ctx);
  for (const InputFill &f : unitFills) {   // the evaluation form of -X^(N/2): two constant halves per limb, the same in every copy
    std::vector<uint64_t> host((size_t)f.addrs.size() * n);
    for (size_t i = 0; i < f.addrs.size(); ++i) {
      const uint64_t q = modulus(f.mods[i]), w = q - hm::powmod(hostP(hostParams).psi.at(f.mods[i]), n / 2, q);
      std::fill(host.begin() + i * n, host.begin() + i * n + n / 2, w);
      std::fill(host.begin() + i * n + n / 2, host.begin() + (i + 1) * n, q - w);
    }
    for (uint32_t c = 0; c < batch_; ++c)
      if (!writeLimbs(f.addrs, host.data(), c)) throw std::runtime_error(std::string("hm_memcpy_h2d (unit): ") + hm_last_error(ctx));
  }
}

static const char *const kLaunchKindNames[] = {"NTT", "INTT", "EWE", "BCONV", "AUTO", "NTT_SUBSCALE", "TENSOR", "EXCH_IN", "EXCH_OUT", "REPLICATE", "IP", "NTT_IP",
                                               "BCONV_COL", "EXCH_IN_COL", "EXCH_OUT_COL", "IP_HOISTED", "IP_LINTRANS", "TENSOR_DOT", "IP_ROTSUM",
                                               "IP_LINTRANS_MULTI", "TENSOR_SQUARE", "LINCOMB", "TENSOR_MULADD", "REIM", "CLINCOMB", "PLINCOMB", "TENSOR_DOTADD",
                                               "LINCOMB_MULTI"};

// Per-launch device time (SURVEY.md §8d "per-stage hipEvent times", exchange time at N > 1): every launch of the plan
// bracketed by its own event pair, in plan order so that the data dependencies (and, sharded, the collectives) line up.
std::string Arch::stageTimes(uint32_t iters) {
  if (!prepared) prepare();
  if (backendKind != BACKEND_HIP) return "";
  std::vector<uint64_t> total(launches.size(), 0);
  for (uint32_t it = 0; it < iters; ++it)
    for (size_t i = 0; i < launches.size(); ++i) {
      hm_timer_start(ctx);
      enqueue(*launches[i]);
      if (launches[i]->recordSlot >= 0) hm_exchange_wait(ctx, (uint32_t)launches[i]->recordSlot);   // timed alone: the compute stream's timer covers the exchange
      uint64_t ns = 0;
      hm_timer_stop(ctx, &ns);
      total[i] += ns;
    }
  std::string out;
  for (size_t i = 0; i < launches.size(); ++i)
    out += std::string(kLaunchKindNames[launches[i]->kind]) + " " + launches[i]->name + " " + std::to_string(total[i] / (iters ? iters : 1)) + "\n";
  return out;
}

std::string Arch::planText() const {
  const char *const *names = kLaunchKindNames;
  std::string out;
  for (const auto &l : launches) {
    size_t cnt = l->out.size();
    if (l->kind == Launch::L_BCONV || l->kind == Launch::L_BCONV_COL) { cnt = 0; for (auto &q : l->probs) cnt += q.out.size(); }
    if (l->kind == Launch::L_IP || l->kind == Launch::L_NTT_IP || l->kind == Launch::L_IP_HOISTED || l->kind == Launch::L_IP_LINTRANS ||
        l->kind == Launch::L_IP_ROTSUM || l->kind == Launch::L_IP_LINTRANS_MULTI)
      cnt = l->mods.size();
    out += std::string(names[l->kind]) + " " + l->name + " n=" + std::to_string(cnt) + " ref=" + std::to_string(l->refInstructions);
    // pass 11: limb-polys an inverse transform stores split-30 packed / conversions (separate or inside a transform's first pass) that read packed inputs
    const size_t po = (size_t)std::count(l->outPacked.begin(), l->outPacked.end(), 1), pi = (size_t)std::count_if(l->probs.begin(), l->probs.end(), [](const Launch::Prob &q) { return q.inPacked; });
    if (po) out += " packed_out=" + std::to_string(po);
    if (pi) out += " packed_in=" + std::to_string(pi) + "/" + std::to_string(l->probs.size());
    if (l->secondOnly) out += " second_pass_only";
    // pass 12: limb-polys whose input (INTT) / addend (fused forward transform) is read through an automorphism
    for (const auto *gv : {&l->inGalois, &l->addGalois}) {
      uint32_t cnt = 0, g = 0;
      for (uint32_t x : *gv) if (x > 1) { ++cnt; g = x; }
      if (cnt) out += std::string(gv == &l->inGalois ? " auto_in=" : " auto_addend=") + std::to_string(cnt) + "/g" + std::to_string(g);
    }
    if (l->xGalois) out += " auto_x=g" + std::to_string(l->xGalois);
    if (!l->mulB.empty()) out += " mul=1";   // pass 4p: the input (INTT) / the minuend (fused forward transform) is a product formed while loading
    if (!l->liftMods.empty()) out += " lift=1";   // ModRaise: the stored input is of another modulus, centred and reduced into the entry's own while loading
    if (!l->hoistG.empty()) {   // (6h): rotations of the hoisted key product and their elements
      out += " rot=" + std::to_string(l->hoistG.size()) + " g=";
      for (size_t r = 0; r < l->hoistG.size(); ++r) out += (r ? "," : "") + std::to_string(l->hoistG[r]);
    }
    if (l->kind == Launch::L_TENSOR_DOT) out += " terms=" + std::to_string(l->dotTerms);   // (5d): pairs summed per record
    if (l->kind == Launch::L_TENSOR_SQUARE)   // (5q): what the records absorbed
      out += std::string(" scale=") + (l->k.empty() ? "0" : "1") + " const=" + (l->addK.empty() ? "0" : "1");
    if (l->kind == Launch::L_LINCOMB)   // (5l): terms summed per record, and whether a constant follows
      out += " terms=" + std::to_string(l->dotTerms) + " const=" + (l->addK.empty() ? "0" : "1");
    if (l->kind == Launch::L_LINCOMB_MULTI)   // (5L): terms and sums per record, and whether constants follow
      out += " terms=" + std::to_string(l->dotTerms) + " out=" + std::to_string(l->multiOuts) + " const=" + (l->addK.empty() ? "0" : "1");
    if (l->kind == Launch::L_CLINCOMB)   // (5c): terms summed per record, and whether a constant follows
      out += " terms=" + std::to_string(l->dotTerms) + " const=" + (l->addK.empty() ? "0" : "1");
    if (l->kind == Launch::L_PLINCOMB)   // (5p): terms summed per record, and whether a plaintext addend follows
      out += " terms=" + std::to_string(l->dotTerms) + " addend=" + (l->d.empty() ? "0" : "1");
    if (l->kind == Launch::L_TENSOR_MULADD)   // (5m): addends per record, and what the records absorbed
      out += " addends=" + std::to_string(l->maAddends) + " scale=" + (l->k.empty() ? "0" : "1") + " const=" + (l->addK.empty() ? "0" : "1");
    if (l->kind == Launch::L_TENSOR_DOTADD)   // (5a): pairs and addends per record, and what the records absorbed
      out += " terms=" + std::to_string(l->dotTerms) + " addends=" + std::to_string(l->maAddends) + " scale=" + (l->k.empty() ? "0" : "1") + " const=" + (l->addK.empty() ? "0" : "1");
    if (l->kind == Launch::L_IP_LINTRANS)   // (6l): entries that also form the addend output
      out += " addend=" + std::to_string(l->d.size() - (size_t)std::count(l->d.begin(), l->d.end(), HM_NO_LIMB));
    if (l->kind == Launch::L_IP_LINTRANS_MULTI)   // (6m): groups, entries that also form the groups' addend outputs
      out += " out=" + std::to_string(l->multiOuts) + " addend=" + std::to_string(l->d.size() - (size_t)std::count(l->d.begin(), l->d.end(), HM_NO_LIMB));
    if ((l->kind == Launch::L_IP_LINTRANS || l->kind == Launch::L_IP_LINTRANS_MULTI) && !l->d1.empty()) out += " id=1";   // ... with the identity step
    if (l->kind == Launch::L_IP_ROTSUM)   // (6s): entries that also form the addend output
      out += " addend=" + std::to_string(l->out1.size() - (size_t)std::count(l->out1.begin(), l->out1.end(), HM_NO_LIMB)) + (l->c.empty() ? "" : " init=1");
    if (l->recordSlot >= 0) out += " mark=" + std::to_string(l->recordSlot);
    if (!l->waitSlots.empty()) { out += " wait="; for (int w : l->waitSlots) out += std::to_string(w) + ","; }
    if (!l->exLimbs.empty()) {
      out += " limbs=";
      for (size_t i = 0; i < l->exLimbs.size(); ++i) out += std::to_string(l->exLimbs[i]) + ":" + std::to_string(l->exOwners[i]) + ",";
    }
    out += "\n";
  }
  return out;
}

// Every field of every launch that enqueue() or replicateForBatch() consumes, one line per launch in launch order (the plan fingerprints of
// tests/test_host_plan_fingerprint.py hash this text).  Deterministic: no pointer is printed, xin / xout appear as launch indices.
std::string Arch::planDump() const {
  std::string out;
  auto vec = [&out](const char *name, const auto &v) {
    if (v.empty()) return;
    out += std::string(" ") + name + "=";
    for (size_t i = 0; i < v.size(); ++i) out += (i ? "," : "") + std::to_string(v[i]);
  };
  auto indexOf = [this](const Launch *x) {
    for (size_t i = 0; i < launches.size(); ++i)
      if (launches[i].get() == x) return std::to_string(i);
    return std::string(x ? "?" : "-");
  };
  for (const auto &l : launches) {
    out += std::string(kLaunchKindNames[l->kind]) + " " + l->name + " stat=" + l->statKey + " opcode=" + std::to_string(l->opcode) + " galois=" + std::to_string(l->galois) +
           " logLen=" + std::to_string(l->logLen) + " secondOnly=" + std::to_string(l->secondOnly) + " hasK=" + std::to_string(l->hasK) + " xGalois=" + std::to_string(l->xGalois) +
           " ipTerms=" + std::to_string(l->ipTerms) + " ipOuts=" + std::to_string(l->ipOuts) + " ref=" + std::to_string(l->refInstructions) + " bytes=" + std::to_string(l->bytes) +
           " mark=" + std::to_string(l->recordSlot) + " xin=" + indexOf(l->xin) + " xout=" + indexOf(l->xout);
    if (l->dotTerms) out += " terms=" + std::to_string(l->dotTerms);
    if (l->kind == Launch::L_TENSOR_MULADD || l->kind == Launch::L_TENSOR_DOTADD) out += " addends=" + std::to_string(l->maAddends);
    if (l->kind == Launch::L_IP_LINTRANS_MULTI || l->kind == Launch::L_LINCOMB_MULTI) out += " multiOuts=" + std::to_string(l->multiOuts);   // (one sum: the line of L_IP_LINTRANS has no such field)
    vec("wait", l->waitSlots); vec("hoistG", l->hoistG); vec("ipCoeff", l->ipCoeff); vec("ipInv", l->ipInv); vec("outPacked", l->outPacked);
    vec("inGalois", l->inGalois); vec("addGalois", l->addGalois); vec("mulB", l->mulB); vec("liftMods", l->liftMods);
    vec("idPt", l->idPt); vec("d1", l->d1);
    vec("a", l->a); vec("b", l->b); vec("c", l->c); vec("d", l->d); vec("out", l->out); vec("out1", l->out1); vec("out2", l->out2);
    vec("mods", l->mods); vec("inMods", l->inMods); vec("k", l->k); vec("mixK", l->mixK); vec("addK", l->addK);
    vec("x0", l->x0); vec("x1", l->x1); vec("maK", l->maK);
    vec("exLimbs", l->exLimbs); vec("exOwners", l->exOwners);
    for (const Launch::Prob &q : l->probs) {
      out += " prob{epi=" + std::to_string(q.epi) + " epAdd=" + std::to_string(q.epAdd) + " inPacked=" + std::to_string(q.inPacked);
      vec("in", q.in); vec("inMods", q.inMods); vec("out", q.out); vec("outMods", q.outMods); vec("epA", q.epA); vec("epB", q.epB); vec("epK", q.epK);
      out += "}";
    }
    out += "\n";
  }
  return out;
}

void Arch::enqueue(Launch &l) {
  hm_status st = HM_OK;
  for (int sl : l.waitSlots)
    if (hm_exchange_wait(ctx, (uint32_t)sl) != HM_OK) throw std::runtime_error("stage " + l.name + ": " + hm_last_error(ctx));
  const uint32_t cnt = (uint32_t)l.out.size();
  std::vector<hm_bconv_desc> descs;
  switch (l.kind) {
  case Launch::L_NTT:
    if (!l.liftMods.empty()) {   // ModRaise: the inputs are stored limb-polys of other moduli
      const hm_ntt_lift_desc m = {hm_ntt_desc{pool, l.a.data(), pool, l.out.data(), l.mods.data(), cnt, 0, nullptr, 0, nullptr, nullptr}, l.liftMods.data()};
      st = hm_ntt_lift(ctx, &m);
    } else {
      st = hm_ntt(ctx, pool, l.a.data(), pool, l.out.data(), l.mods.data(), cnt, 0, nullptr);
    }
    break;
  case Launch::L_INTT: {
    const bool anyPacked = std::find(l.outPacked.begin(), l.outPacked.end(), 1) != l.outPacked.end();
    hm_ntt_desc d = {pool, l.a.data(), pool, l.out.data(), l.mods.data(), cnt, 1, l.hasK ? l.k.data() : nullptr, l.secondOnly ? 1 : 0,
                     anyPacked ? l.outPacked.data() : nullptr, l.inGalois.empty() ? nullptr : l.inGalois.data()};
    if (!l.mulB.empty()) {   // (4p): the inputs are products
      const hm_ntt_mul_desc m = {d, pool, l.mulB.data()};
      st = hm_ntt_mul(ctx, &m);
    } else {
      st = hm_ntt_ex(ctx, &d);
    }
    break;
  }
  case Launch::L_NTT_SUBSCALE:
    if (!l.mixK.empty() || !l.probs.empty() || !l.addGalois.empty() || !l.mulB.empty()) {
      for (auto &q : l.probs)
        descs.push_back(hm_bconv_desc{pool, q.in.data(), q.inMods.data(), (uint32_t)q.in.size(), pool, q.out.data(), q.outMods.data(), (uint32_t)q.out.size(), 0,
                                    nullptr, nullptr, nullptr, nullptr, nullptr, q.inPacked ? 1u : 0u});
      hm_ntt_fused_desc d = {pool, l.a.data(), l.mixK.empty() ? nullptr : pool, l.mixK.empty() ? nullptr : l.d.data(), l.mixK.empty() ? nullptr : l.mixK.data(), pool, l.b.data(),
                             l.c.empty() ? nullptr : pool, l.c.empty() ? nullptr : l.c.data(), l.addK.empty() ? nullptr : l.addK.data(), pool, l.out.data(), l.mods.data(), cnt,
                             l.k.data(), descs.empty() ? nullptr : descs.data(), (uint32_t)descs.size(), l.addGalois.empty() ? nullptr : l.addGalois.data()};
      if (!l.mulB.empty()) {   // (4p): the minuends are products
        const hm_ntt_fused_mul_desc m = {d, pool, l.mulB.data()};
        st = hm_ntt_mix_sub_scale_mul(ctx, &m);
      } else {
        st = hm_ntt_mix_sub_scale(ctx, &d);
      }
    } else {
      st = hm_ntt_sub_scale(ctx, pool, l.a.data(), pool, l.b.data(), l.c.empty() ? nullptr : pool, l.c.empty() ? nullptr : l.c.data(), pool,
                            l.out.data(), l.mods.data(), cnt, l.k.data());
    }
    break;
  case Launch::L_IP: {
    const hm_ip_desc d = {pool, l.a.data(), pool, l.b.data(), pool, l.out.data(), l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms, l.ipOuts, l.xGalois};
    st = hm_inner_product_ex(ctx, &d);
    break;
  }
  case Launch::L_IP_HOISTED: {
    const hm_ip_hoisted_desc d = {pool, l.a.data(), pool, l.b.data(), pool, l.out.data(), l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms,
                                  (uint32_t)l.hoistG.size(), l.hoistG.data()};
    st = hm_inner_product_hoisted(ctx, &d);
    break;
  }
  case Launch::L_IP_LINTRANS: {
    const bool add = !l.d.empty();
    if (!l.d1.empty()) {   // the identity step: the several-sums form with one sum (the same limb lists)
      const hm_ip_lintrans_id_desc d = {{pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), pool, l.d.data(), pool, l.out.data(), pool, l.out1.data(),
                                         l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms, (uint32_t)l.hoistG.size(), 1, l.hoistG.data()},
                                        l.idPt.data(), pool, l.d1.data(), pool, l.out2.data()};
      st = hm_inner_product_lintrans_id(ctx, &d);
      break;
    }
    const hm_ip_lintrans_desc d = {pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), add ? pool : nullptr, add ? l.d.data() : nullptr, pool, l.out.data(),
                                   add ? pool : nullptr, add ? l.out1.data() : nullptr, l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms,
                                   (uint32_t)l.hoistG.size(), l.hoistG.data()};
    st = hm_inner_product_lintrans(ctx, &d);
    break;
  }
  case Launch::L_IP_LINTRANS_MULTI: {
    const bool add = !l.d.empty();
    if (!l.d1.empty()) {
      const hm_ip_lintrans_id_desc d = {{pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), pool, l.d.data(), pool, l.out.data(), pool, l.out1.data(),
                                         l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms, (uint32_t)l.hoistG.size(), l.multiOuts, l.hoistG.data()},
                                        l.idPt.data(), pool, l.d1.data(), pool, l.out2.data()};
      st = hm_inner_product_lintrans_id(ctx, &d);
      break;
    }
    const hm_ip_lintrans_multi_desc d = {pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), add ? pool : nullptr, add ? l.d.data() : nullptr, pool,
                                         l.out.data(), add ? pool : nullptr, add ? l.out1.data() : nullptr, l.mods.data(), (uint32_t)l.mods.size(),
                                         l.ipTerms, (uint32_t)l.hoistG.size(), l.multiOuts, l.hoistG.data()};
    st = hm_inner_product_lintrans_multi(ctx, &d);
    break;
  }
  case Launch::L_IP_ROTSUM: {
    const bool add = !l.d.empty();
    if (!l.c.empty()) {   // with initial sums
      const hm_ip_rotsum_init_desc d = {{pool, l.a.data(), pool, l.b.data(), add ? pool : nullptr, add ? l.d.data() : nullptr, pool, l.out.data(),
                                         add ? pool : nullptr, add ? l.out1.data() : nullptr, l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms,
                                         (uint32_t)l.hoistG.size(), l.hoistG.data()},
                                        pool, l.c.data(), add ? l.d1.data() : nullptr};
      st = hm_inner_product_rotsum_init(ctx, &d);
      break;
    }
    const hm_ip_rotsum_desc d = {pool, l.a.data(), pool, l.b.data(), add ? pool : nullptr, add ? l.d.data() : nullptr, pool, l.out.data(),
                                 add ? pool : nullptr, add ? l.out1.data() : nullptr, l.mods.data(), (uint32_t)l.mods.size(), l.ipTerms,
                                 (uint32_t)l.hoistG.size(), l.hoistG.data()};
    st = hm_inner_product_rotsum(ctx, &d);
    break;
  }
  case Launch::L_NTT_IP: {
    for (auto &q : l.probs)
      descs.push_back(hm_bconv_desc{pool, q.in.data(), q.inMods.data(), (uint32_t)q.in.size(), pool, q.out.data(), q.outMods.data(), (uint32_t)q.out.size(), 0,
                                    nullptr, nullptr, nullptr, nullptr, nullptr, q.inPacked ? 1u : 0u});
    hm_ntt_ip_desc d = {pool, l.a.data(), l.ipCoeff.data(), pool, l.c.data(), pool, l.b.data(), pool, l.out.data(), l.mods.data(),
                        (uint32_t)l.mods.size(), l.ipTerms, l.ipOuts, descs.empty() ? nullptr : descs.data(), (uint32_t)descs.size(),
                        std::find(l.ipInv.begin(), l.ipInv.end(), 1) != l.ipInv.end() ? l.ipInv.data() : nullptr, l.xGalois};
    st = hm_ntt_inner_product(ctx, &d);
    break;
  }
  case Launch::L_TENSOR:
    st = hm_tensor(ctx, pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), pool, l.d.data(), pool, l.out.data(), pool, l.out1.data(), pool,
                   l.out2.data(), l.mods.data(), cnt);
    break;
  case Launch::L_TENSOR_DOT:
    st = hm_tensor_dot(ctx, pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), pool, l.d.data(), pool, l.out.data(), pool, l.out1.data(), pool,
                       l.out2.data(), l.mods.data(), cnt, l.dotTerms);
    break;
  case Launch::L_TENSOR_SQUARE:
    st = hm_tensor_square(ctx, pool, l.a.data(), pool, l.c.data(), pool, l.out.data(), pool, l.out1.data(), pool, l.out2.data(), l.mods.data(), cnt,
                          l.k.empty() ? nullptr : l.k.data(), l.addK.empty() ? nullptr : l.addK.data());
    break;
  case Launch::L_LINCOMB:
    st = hm_lincomb(ctx, pool, l.a.data(), pool, l.out.data(), l.mods.data(), cnt, l.dotTerms, l.k.data(), l.addK.empty() ? nullptr : l.addK.data());
    break;
  case Launch::L_LINCOMB_MULTI:
    st = hm_lincomb_multi(ctx, pool, l.a.data(), pool, l.out.data(), l.mods.data(), (uint32_t)l.mods.size(), l.dotTerms, l.multiOuts, l.k.data(),
                          l.addK.empty() ? nullptr : l.addK.data());
    break;
  case Launch::L_TENSOR_MULADD:
    st = hm_tensor_muladd(ctx, pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), pool, l.d.data(), l.maAddends ? pool : nullptr,
                          l.maAddends ? l.x0.data() : nullptr, l.maAddends ? l.x1.data() : nullptr, pool, l.out.data(), pool, l.out1.data(), pool,
                          l.out2.data(), l.mods.data(), cnt, l.maAddends, l.k.empty() ? nullptr : l.k.data(), l.maAddends ? l.maK.data() : nullptr,
                          l.addK.empty() ? nullptr : l.addK.data());
    break;
  case Launch::L_REIM:
    st = hm_reim_split(ctx, pool, l.a.data(), pool, l.c.data(), pool, l.out.data(), pool, l.out1.data(), l.mods.data(), cnt);
    break;
  case Launch::L_CLINCOMB:
    st = hm_clincomb(ctx, pool, l.a.data(), pool, l.out.data(), l.mods.data(), cnt, l.dotTerms, l.k.data(), l.maK.data(),
                     l.addK.empty() ? nullptr : l.addK.data(), nullptr);
    break;
  case Launch::L_PLINCOMB:
    st = hm_plincomb(ctx, pool, l.b.data(), pool, l.x0.data(), l.x1.data(), l.d.empty() ? nullptr : pool, l.d.empty() ? nullptr : l.d.data(), pool,
                     l.out.data(), l.out1.data(), l.mods.data(), cnt, l.dotTerms);
    break;
  case Launch::L_TENSOR_DOTADD:
    st = hm_tensor_dotadd(ctx, pool, l.a.data(), pool, l.b.data(), pool, l.c.data(), pool, l.d.data(), l.maAddends ? pool : nullptr,
                          l.maAddends ? l.x0.data() : nullptr, l.maAddends ? l.x1.data() : nullptr, pool, l.out.data(), pool, l.out1.data(), pool,
                          l.out2.data(), l.mods.data(), cnt, l.dotTerms, l.maAddends, l.k.empty() ? nullptr : l.k.data(),
                          l.maAddends ? l.maK.data() : nullptr, l.addK.empty() ? nullptr : l.addK.data());
    break;
  case Launch::L_EXCH_IN:
    st = hm_limbs_to_slices(ctx, pool, l.exLimbs.data(), l.exOwners.data(), (uint32_t)l.exLimbs.size(), l.slicesIn);
    break;
  case Launch::L_EXCH_OUT:
    st = hm_slices_to_limbs(ctx, l.slicesOut, pool, l.exLimbs.data(), l.exOwners.data(), (uint32_t)l.exLimbs.size());
    break;
  case Launch::L_EXCH_IN_COL:
    st = hm_limbs_to_colslices(ctx, pool, l.exLimbs.data(), l.exOwners.data(), (uint32_t)l.exLimbs.size(), l.slicesIn);
    break;
  case Launch::L_EXCH_OUT_COL:
    st = hm_colslices_to_limbs(ctx, l.slicesOut, pool, l.exLimbs.data(), l.exOwners.data(), (uint32_t)l.exLimbs.size());
    break;
  case Launch::L_BCONV_COL:
    for (auto &q : l.probs)
      descs.push_back(hm_bconv_desc{l.slicesIn, q.in.data(), q.inMods.data(), (uint32_t)q.in.size(), l.slicesOut, q.out.data(), q.outMods.data(), (uint32_t)q.out.size(), 0});
    st = hm_bconv_col(ctx, descs.data(), (uint32_t)descs.size(), l.galois, l.logLen);
    break;
  case Launch::L_REPLICATE:
    st = hm_replicate_limbs(ctx, pool, l.exLimbs.data(), l.exOwners.data(), (uint32_t)l.exLimbs.size());
    break;
  case Launch::L_AUTO:
    st = hm_automorph(ctx, pool, l.a.data(), pool, l.out.data(), cnt, l.galois);
    break;
  case Launch::L_EWE:
    st = hm_ewe(ctx, l.opcode, pool, l.a.data(), pool, l.b.empty() ? nullptr : l.b.data(), pool, l.c.empty() ? nullptr : l.c.data(), pool,
                l.d.empty() ? nullptr : l.d.data(), pool, l.out.data(), l.mods.data(), cnt, l.hasK ? l.k.data() : nullptr);
    break;
  case Launch::L_BCONV:
    for (auto &q : l.probs)
      descs.push_back(hm_bconv_desc{l.slicesIn ? l.slicesIn : pool, q.in.data(), q.inMods.data(), (uint32_t)q.in.size(),
                                    l.slicesOut ? l.slicesOut : pool, q.out.data(), q.outMods.data(), (uint32_t)q.out.size(), l.logLen,
                                    q.epi ? pool : nullptr, q.epi ? q.epA.data() : nullptr, q.epAdd ? pool : nullptr, q.epAdd ? q.epB.data() : nullptr,
                                    q.epi ? q.epK.data() : nullptr, q.inPacked ? 1u : 0u});
    st = hm_bconv_batch(ctx, descs.data(), (uint32_t)descs.size());
    break;
  }
  if (st == HM_OK && l.recordSlot >= 0) st = hm_exchange_mark(ctx, (uint32_t)l.recordSlot);
  if (st != HM_OK) throw std::runtime_error("stage " + l.name + ": " + hm_last_error(ctx));
}

void Arch::update() {
  if (backendKind == BACKEND_SIM) {
    if (!sim) throw std::runtime_error("sim backend: no program loaded");
    sim->step();
    return;
  }
  if (!prepared) prepare();
  if (nextLaunch >= launches.size()) return;
  Launch &l = *launches[nextLaunch++];
  if (backendKind == BACKEND_HIP) {
    hm_timer_start(ctx);
    enqueue(l);
    if (l.recordSlot >= 0) hm_exchange_wait(ctx, (uint32_t)l.recordSlot);
    uint64_t ns = 0;
    hm_timer_stop(ctx, &ns);
    elapsedNs += ns;
    stat->increaseStat(l.statKey + "_(0)", ns);  // per-unit busy time, ns (upstream: busy cycles per cluster)
  }
  stat->increaseStat(l.statKey + "_launches");
  completedIns += l.refInstructions;
}

bool Arch::simulateComplete() { return sim ? sim->complete() : prepared && nextLaunch >= launches.size(); }
unsigned long long Arch::getCycle() { return sim ? sim->cycle() : elapsedNs; }
unsigned long long Arch::getcompletedIns() { return sim ? sim->completedIns() : completedIns; }

void Arch::state() {
  if (sim) { std::cout << sim->describe(); return; }
  std::cout << "launched " << nextLaunch << " of " << launches.size() << " stages\n";
  if (nextLaunch < launches.size()) std::cout << "next: " << launches[nextLaunch]->name << "\n";
}

void Arch::shownStat() {
  if (sim) {  // the reference's block: same keys, same order (std::map), same values
    std::cout << "Start outPut statistic informations:\n";
    std::cout << "=====================================\n";
    for (const auto &kv : sim->stats()) std::cout << kv.first << " :\t" << kv.second << "\n";
    return;
  }
  stat->setStat("Total_ns", elapsedNs);
  // measured HBM bytes of the op from the profiler ("rocprof HBM counters in the same key : value block"; upstream's
  // HBM_(c) / MEM_(c) counters, src/mem.cpp:68-69,105-107).  A process cannot read its own rocprofv3 counters: the figures come from
  // the counter file a profiling pass left (profiles/roofline_inputs.json, written by tools/make_roofline_inputs.py), named by
  // HOMULATOR_COUNTER_FILE, and are printed only if that file describes this launch shape (hmult at N = 2^16 with this batch).
  if (const char *path = getenv("HOMULATOR_COUNTER_FILE")) {
    std::ifstream f(path);
    std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    auto num = [&](const std::string &key, double &v) {
      size_t p = text.find("\"" + key + "\"");
      if (p == std::string::npos) return false;
      p = text.find(':', p);
      if (p == std::string::npos) return false;
      v = atof(text.c_str() + p + 1);
      return true;
    };
    double fetch = 0, write = 0, b = 0;
    if (num("whole_op_fetch_kib", fetch) && num("whole_op_write_kib", write) && num("whole_op_batch", b) && (uint32_t)b == batch_ && n == 65536 && maxLevel_ == 45 && curLevel_ == 35 &&
        std::any_of(launches.begin(), launches.end(), [](const std::unique_ptr<Launch> &l) { return l->kind == Launch::L_TENSOR; })) {
      stat->setStat("HBM_fetch_KiB_per_op", (unsigned long long)(2 * fetch));   // FETCH_SIZE counts 64 B per 128-B request on gfx950
      stat->setStat("HBM_write_KiB_per_op", (unsigned long long)write);
      stat->setStat("HBM_bytes_per_op", (unsigned long long)((2 * fetch + write) * 1024));
    }
  }
  stat->showStat();
}

void Arch::run() {
  if (backendKind != BACKEND_HIP) return;
  for (Binding &b : bindings) {  // stream-ordered after the producer; one gather-copy launch per bound ciphertext part
    if (hm_wait_for(ctx, b.src->ctx) != HM_OK) throw std::runtime_error(std::string("hm_wait_for: ") + hm_last_error(ctx));
    if (hm_ewe(ctx, EWE_COPY, b.src->pool, b.srcLimbs.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, pool, b.dstLimbs.data(),
               b.mods.data(), (uint32_t)b.dstLimbs.size(), nullptr) != HM_OK)
      throw std::runtime_error(std::string("bound input copy: ") + hm_last_error(ctx));
    // back edge: the producer's NEXT pass overwrites these limbs (its transforms even use their output as first-pass
    // scratch), so its stream waits until this copy has read them
    if (hm_wait_for(b.src->ctx, ctx) != HM_OK) throw std::runtime_error(std::string("hm_wait_for (back edge): ") + hm_last_error(ctx));
  }
  // single GPU: the plan is a fixed sequence of kernels -> captured into a HIP graph on the second run (the first
  // one warms the base-conversion table cache, which allocates) and replayed with one launch afterwards.
  // Sharded runs enqueue directly: the RCCL groups stay outside graphs.
  if (useGraph && world_ == 1) {
    if (graph) {
      if (hm_graph_launch(ctx, static_cast<hm_graph *>(graph)) != HM_OK) throw std::runtime_error(std::string("hm_graph_launch: ") + hm_last_error(ctx));
      return;
    }
    if (runCount++ >= 1) {
      hm_graph *g = nullptr;
      if (hm_capture_begin(ctx) != HM_OK) throw std::runtime_error(std::string("hm_capture_begin: ") + hm_last_error(ctx));
      for (auto &l : launches) enqueue(*l);
      if (hm_capture_end(ctx, &g) != HM_OK) throw std::runtime_error(std::string("hm_capture_end: ") + hm_last_error(ctx));
      graph = g;
      if (hm_graph_launch(ctx, g) != HM_OK) throw std::runtime_error(std::string("hm_graph_launch: ") + hm_last_error(ctx));
      return;
    }
  }
  for (auto &l : launches) enqueue(*l);
}
void Arch::sync() {
  if (ctx) hm_sync(ctx);
}
double Arch::timedRun(uint32_t iters) {
  if (!prepared) prepare();
  if (backendKind != BACKEND_HIP) return 0.0;
  hm_timer_start(ctx);
  for (uint32_t i = 0; i < iters; ++i) run();
  uint64_t ns = 0;
  hm_timer_stop(ctx, &ns);
  return (double)ns / iters;
}

void Arch::refill(const std::vector<AddrType> &addrs, uint64_t seed) {
  if (!prepared) prepare();
  if (backendKind != BACKEND_HIP || addrs.empty()) return;
  const InputFill *f = nullptr;
  for (const InputFill &x : fills)
    if (x.addrs == addrs) f = &x;
  if (!f) throw std::runtime_error("refill: not an input of this op");
  for (uint32_t c = 0; c < (f->shared ? 1u : batch_); ++c) {
    std::vector<uint32_t> limbs;
    for (AddrType a : addrs) limbs.push_back(limbOf(a) + c * (uint32_t)limbIndex.size());
    if (hm_fill_uniform(ctx, pool, limbs.data(), f->mods.data(), (uint32_t)limbs.size(), seed + c * kBatchSeedStride) != HM_OK)
      throw std::runtime_error(std::string("hm_fill_uniform: ") + hm_last_error(ctx));
  }
}
void Arch::snapshot(const std::vector<AddrType> &addrs, uint32_t slot) {
  if (!prepared) prepare();
  if (backendKind != BACKEND_HIP) return;
  auto &sn = snapshots[slot];
  if (sn.second != addrs.size()) {
    if (sn.first) hm_free(ctx, sn.first);
    void *p = nullptr;
    if (hm_malloc(ctx, addrs.size() * (size_t)n * 8, &p) != HM_OK) throw std::runtime_error(std::string("hm_malloc (snapshot): ") + hm_last_error(ctx));
    sn = {static_cast<uint64_t *>(p), addrs.size()};
  }
  for (size_t i = 0; i < addrs.size(); ++i)
    if (hm_memcpy_d2d(ctx, sn.first + i * n, pool + (size_t)limbOf(addrs[i]) * n, (size_t)n * 8) != HM_OK)
      throw std::runtime_error(std::string("hm_memcpy_d2d: ") + hm_last_error(ctx));
}
bool Arch::readSnapshot(uint32_t slot, uint64_t *host) {
  auto it = snapshots.find(slot);
  if (it == snapshots.end() || backendKind != BACKEND_HIP) return false;
  return hm_memcpy_d2h(ctx, host, it->second.first, it->second.second * (size_t)n * 8) == HM_OK;
}

// real data in: overwrites limb-polys (inputs, evaluation-key limbs) after prepare(); stream-ordered after everything enqueued so far
bool Arch::writeLimbs(const std::vector<AddrType> &addrs, const uint64_t *host, uint32_t copy) {
  if (backendKind != BACKEND_HIP || !pool || copy >= batch_) return false;
  sync();
  for (size_t i = 0; i < addrs.size(); ++i)
    if (hm_memcpy_h2d(ctx, pool + ((size_t)limbOf(addrs[i]) + (size_t)copy * limbIndex.size()) * n, host + i * n, (size_t)n * 8) != HM_OK) return false;
  return true;
}
void Arch::encodeLimbs(const std::vector<AddrType> &addrs, const std::vector<uint32_t> &mods, const double *slots, double scale, uint32_t copy) {
  if (world_ > 1) throw std::runtime_error("encode_plaintext: not on a sharded plan (world > 1)");
  if (backendKind != BACKEND_HIP) throw std::runtime_error("encode_plaintext: only the hip backend holds values");
  if (!prepared) prepare();
  if (!pool || copy >= batch_) throw std::runtime_error("encode_plaintext: copy " + std::to_string(copy) + " is not an op of the batch");
  auto ck = [&](hm_status st, const char *what) { if (st != HM_OK) throw std::runtime_error(std::string("encode_plaintext: ") + what + ": " + hm_last_error(ctx)); };
  if (!encodeScratch) {
    void *p = nullptr;
    ck(hm_malloc(ctx, 2 * (size_t)n * 8, &p), "hm_malloc");
    encodeScratch = static_cast<uint64_t *>(p);
  }
  const hm::Params &hp = hostP(hostParams);
  uint32_t src = 0;
  for (uint32_t m = 1; m < hp.mod.size(); ++m)
    if (hp.mod[m] > hp.mod[src]) src = m;
  std::vector<uint32_t> limbs;
  for (AddrType a : addrs) limbs.push_back(limbOf(a));
  uint64_t *copyPool = pool + (size_t)copy * limbIndex.size() * n;   // the copy's own base, as writeLimbs: limb numbers stay those of one op
  sync();
  uint64_t stale = 0;
  ck(hm_get_counter(ctx, "encode_overflow", &stale), "hm_get_counter");   // an earlier caller's flag is not this vector's
  ck(hm_memcpy_h2d(ctx, encodeScratch, slots, (size_t)n * 8), "hm_memcpy_h2d");
  const uint32_t workLimb = 1;
  ck(hm_encode(ctx, reinterpret_cast<const double *>(encodeScratch), 1, scale, encodeScratch, &workLimb, src, copyPool, limbs.data(), mods.data(), (uint32_t)mods.size()),
     "hm_encode");
  uint64_t over = 0;
  ck(hm_get_counter(ctx, "encode_overflow", &over), "hm_get_counter");
  if (over) throw std::runtime_error("encode_plaintext: a coefficient exceeds half the largest modulus of the chain at this scale");
}
bool Arch::readLimbs(const std::vector<AddrType> &addrs, uint64_t *host, uint32_t copy) {
  if (backendKind != BACKEND_HIP || !pool || copy >= batch_) return false;
  for (size_t i = 0; i < addrs.size(); ++i)
    if (hm_memcpy_d2h(ctx, host + i * n, pool + ((size_t)limbOf(addrs[i]) + (size_t)copy * limbIndex.size()) * n, (size_t)n * 8) != HM_OK) return false;
  return true;
}
