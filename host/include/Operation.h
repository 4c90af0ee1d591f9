// Operation.h — the FHE operation layer with the reference's class names, constructor signatures and
// simulate() entry (include/Operation.h:18-321): KeySwitch, TensorCompute, Rescale sub-builders and the op
// classes HMULT, HROTATE, HADD, PMULT, PADD, each `ctor(label, maxLevel, curLevel, alpha, Config*, Arch*)`.
// The constructors build the stage graph (same stage keys, same order, same buffer names as upstream's
// src/Operation.cpp) with the mathematically correct wiring of SURVEY.md Appendix A / C; simulate() executes
// it on the backend and prints the upstream banner and stat block.
#ifndef HOMULATOR_OPERATION_H
#define HOMULATOR_OPERATION_H
#include "Addr.h"
#include "Arch.h"
#include "Basic.h"
#include "Context.h"
#include "Driver.h"
#include "InsGen.h"

#include <array>
#include <complex>
#include <deque>

// the stages of one builder: (stage key, [level] -> instruction group) in the order they were emitted, with upstream's lookup by key
class StageList {
  std::deque<std::pair<std::string, std::vector<INSGROUP>>> stages_;  // a deque: what add() returns stays where it is

public:
  std::vector<INSGROUP> &add(const std::string &key, std::vector<INSGROUP> groups) {
    stages_.emplace_back(key, std::move(groups));
    return stages_.back().second;
  }
  const std::vector<INSGROUP> &at(const std::string &key) const {
    for (const auto &s : stages_)
      if (s.first == key) return s.second;
    throw std::out_of_range("no stage " + key);
  }
  auto begin() const { return stages_.begin(); }
  auto end() const { return stages_.end(); }
};

// a buffer as one part of a key switch hands it to the next: its limb addresses and, per limb, the group of the stage that writes it.  The
// consumer depends on these groups and looks up no name.
struct Limbs {
  std::vector<AddrType> addr;
  std::vector<INSGROUP> from;
};

// The key switch in parts, with explicit values between them: modUp -> [rotateDigits ->] keyProduct -> modDown.  Upstream's constructor is the
// whole key switch of its input; the hoisted rotations (HROTATE_HOISTED) run modUp once and the other three parts per rotation, every buffer and
// stage key of a rotation carrying the suffix "_Rot<r>".
class KeySwitch {
public:
  typedef std::vector<Limbs> Digits;                   // per digit j: the E = level + alpha limbs of the extended digit, in evaluation form
  typedef std::array<Limbs, 2> Accumulators;           // per key component k: the E limbs of sum_j digit_j * evk_{j,k}
  typedef std::array<std::vector<AddrType>, 2> Output; // per key component k: the `level` limbs of the switched polynomial

private:
  std::map<AddrType, std::vector<Instruction *>> *DataInsMap;
  InsGen *insGenPointer;
  uint32_t Level, Alpha, Beta, MaxLevel;
  AddrManage *memMange;
  Arch *arch;
  std::string baseName;
  std::vector<uint32_t> qMods, pMods, extMods;  // modulus ids of the `level` Q limbs, of the alpha special primes, and of both (the extended basis)
  StageList stages;
  Output out_;

public:
  KeySwitch(std::string labelName, uint32_t maxlevel, uint32_t level, uint32_t alpha,
            const std::vector<AddrType> &inputPolynomialAddress, std::vector<AddrType> *pool,
            std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen, AddrManage *memoryMange);
  // emits nothing: the caller composes the parts
  KeySwitch(std::string labelName, uint32_t maxlevel, uint32_t level, uint32_t alpha, std::vector<AddrType> *pool,
            std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen, AddrManage *memoryMange);
  const StageList &getInsMap() const { return stages; }
  StageList takeStages() { return std::exchange(stages, StageList()); }  // the stages emitted since the last call
  const Output &output() const { return out_; }                         // of upstream's constructor

  // inputMayBeOpInput: the input may be an op's own input ciphertext, which no instruction produces (otherwise a limb without producer throws)
  // suffix: on every buffer and stage key, for the ops that run more than one ModUp (HROTSUM: "_Ct<i>" from the second ciphertext on; HBSGS:
  // "_Giant<i>" for the intermediate ciphertexts of the giant step)
  Digits modUp(const std::vector<AddrType> &input, bool inputMayBeOpInput, const std::string &suffix = "");
  Digits rotateDigits(const Digits &digits, uint32_t galois, const std::string &suffix);
  Accumulators keyProduct(const Digits &digits, uint64_t keySeed, const std::string &suffix);  // keySeed: the synthetic stream of the key
  Output modDown(const Accumulators &acc, const std::string &suffix);
};

class TensorCompute {
private:
  StageList stages;
  std::array<std::vector<AddrType>, 3> d_;

public:
  // bufferPrefix / bufferSuffix: the outputs are <prefix>D<i>Out<suffix> (upstream: TensorD<i>Out; HDOT names its own)
  TensorCompute(std::string labelName, uint32_t level, Ciphertext *cipher1, Ciphertext *cipher2,
                std::vector<AddrType> *pool, std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen,
                AddrManage *memoryMange, const std::string &bufferPrefix = "Tensor", const std::string &bufferSuffix = "");
  const StageList &getInsMap() const { return stages; }
  const std::vector<AddrType> &d(uint32_t i) const { return d_[i]; }  // TensorD<i>Out
};

class Rescale {
private:
  StageList stages;
  std::vector<AddrType> out_;

public:
  Rescale(std::string labelName, uint32_t level, const std::vector<AddrType> &inputPolynomialAddress,
          std::vector<AddrType> *pool, std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen,
          AddrManage *memoryMange, bool inputMayBeOpInput = false);   // inputMayBeOpInput: as KeySwitch::modUp's (HRESCALE)
  const StageList &getInsMap() const { return stages; }
  const std::vector<AddrType> &output() const { return out_; }  // <base>_Rescale_MulOut
};

// common part of the op classes: generators, driver, address plan, synthetic inputs, simulate()
class OperationBase {
protected:
  std::vector<AddrType> Datapool;
  std::map<AddrType, std::vector<Instruction *>> DataInsMap;  // owns the instructions (freed by the destructor)
  InsGen insgener;
  Driver driver;
  std::unique_ptr<AddrManage> addrManager;  // made by makeInputs(): the temporaries start after the inputs
  std::vector<Ciphertext> cts;              // the input ciphertexts ct1, ct2, ... (HDOT: ct1 .. ct<2T>, HROTSUM: ct1 .. ct<G>)
  std::unique_ptr<Plaintext> ptx;           // the input plaintext pt
  std::vector<Plaintext> levelPtx;          // the input plaintexts pt1, pt2, ... (pt0) of `level` limbs on the ciphertext basis (HPLINCOMB)
  std::vector<Plaintext> extPtx;            // the input plaintexts pt1, pt2, ... on the extended basis (HLINTRANS; HBSGS: pt<(i-1)R+r>)
  Arch *arch;
  Config *config;
  std::string opName;       // HMULT, HROTATE, ...
  std::string label;        // constructor label ("test_hmult", ...): part of the rescale buffer names
  uint32_t maxLevel_, level_, alpha_;
  uint32_t batchSize, N;
  uint64_t seed;
  std::map<std::string, std::vector<AddrType>> namedInputs;   // ct1.c0, ct1.c1, ... for readBuffer
  std::map<std::string, std::vector<AddrType>> namedOutputs;  // out.c0, out.c1
  std::map<std::string, std::vector<uint32_t>> plaintextMods;  // the input plaintexts by name (pt, pt<r>, pt0, ...): the modulus of every limb, for encodePlaintext

  OperationBase(const std::string &op, const std::string &labelName, Config *cfg, Arch *_arch, uint32_t maxLevel, uint32_t curLevel, uint32_t alpha);
  // every op's preamble: `ciphertexts` input ciphertexts ct1, ct2 (synthetic streams seed, seed + 2000) and, if asked, the plaintext pt
  // (seed + 4000) at the current level, then `extPlaintexts` plaintexts pt<r>, r = 1.., on the extended basis (the current level's Q limbs, then
  // the alpha special primes; seed + 4000 + 100000 r), then the named extra plaintexts `namedExt` on the extended basis too ((name, stream): seed +
  // stream; the identity step's pt0), then the address plan of the temporaries behind them
  typedef std::vector<std::pair<std::string, uint64_t>> NamedStreams;
  // namedLevel: plaintexts of `level` limbs on the ciphertext basis, by name and stream (HPLINCOMB), behind everything else
  void makeInputs(uint32_t ciphertexts, bool plaintext = false, uint32_t extPlaintexts = 0, const NamedStreams &namedExt = {}, const NamedStreams &namedLevel = {});
  // config key `identity` (0 or 1, default 0; read by the ops that have an identity step): the unrotated diagonal, DESIGN.md section 16
  bool identityStep(const std::string &op) const;
  // what the ops that hoist the ModUp over rotations (HROTATE_HOISTED, HLINTRANS, HBSGS) or sum rotations in front of one ModDown (HROTSUM) check
  // first (`op` names the op in the messages): no backend = sim,
  // no world > 1; config keys `rotations` = R (default 4, 1..16) and `galois` = g (default 5, odd, below 2N).  Returns g^r mod 2N, r = 1..R, distinct
  std::vector<uint32_t> hoistedRotations(const std::string &op) const;
  // config key `rescale` (0 or 1, default 0; read by PMULT, HLINTRANS, HROTSUM, HBSGS): the op's result goes through Rescale, DESIGN.md section 17
  bool rescaleKey(const std::string &op) const;
  // <out>.c<k> = Rescale(ct[k]), builder labels <label>_<k>, as HMULT's tail: the tail of the ops with rescale = 1, and all of HRESCALE
  void setRescaledOutput(const std::string &out, const std::array<std::vector<AddrType>, 2> &ct, bool inputMayBeOpInput = false);
  // HMULT's tail on the three polynomials d of a tensor product (shared by HMULT, HDOT, HSQUARE, HMULADD, HDOTADD): KS(d[2]); HMULT_Hadd_Key(k): d[k] + ks_k into
  // HMULTHaddOutput(k); Rescale of both, out = the result at level - 1
  void relinearizeAndRescale(const std::array<std::vector<AddrType>, 3> &d);
  // Per-limb constants an op carries in its records (HSQUARE: "scale", "const"; HLINCOMB: "scale<t>", "const"; HMLINCOMB: "scale<m>_<t>", "const<m>"; HCLINCOMB: "scale<t>", "scale_im<t>", "const"; HMULADD: "scale", "addscale<t>", "const"; HDOTADD: "scale<t>", "addscale<r>", "const"), by name: the records of limb j that hold value j, so that
  // setConstants can patch Instruction::constant before the plan is built.  enabled = false: the op knows the name but its config key is 0
  // negated: the records carry q_j - value (HCLINCOMB's "scale_im<t>": the stage multiplies by the stored -X^(N/2))
  struct ConstantStage { bool enabled = false; std::string key; std::vector<std::vector<Instruction *>> records; bool nonZero = false; bool negated = false; };
  std::map<std::string, ConstantStage> constantStages;
  // ---- what the builders of the fused element-wise ops share (HREIM, HDOT .. HDOTADD).  `op` names the op in the messages
  // a build extension has no backend = sim ("... has no such op (<why>)") and no world > 1
  void refuseSimAndSharded(const std::string &op, const std::string &why) const;
  bool flag(const std::string &op, const char *key, uint32_t dflt = 0) const;   // a config key that is 0 or 1
  uint32_t countKey(const std::string &op, const char *key, uint32_t dflt, uint32_t lo, uint32_t hi) const;   // ... in [lo, hi] (terms, addends, outputs)
  // per-limb constants from the synthetic stream `stream` (word 0 of limb j's stream); nonZero: 1 in place of 0 (a constant that multiplies);
  // negated: q_j - value
  std::vector<uint64_t> synth(uint64_t stream, bool nonZero = false, bool negated = false) const;
  // the records of limb j of a constant stage (one group per limb), kept under `name` for setConstants
  void keep(const std::string &name, const std::vector<INSGROUP> &recs, bool nonZero = false, bool negated = false);
  // one element-wise stage over the `level` limbs, stage key `key`, labels <label>_<key>_Level(j), into the new buffer `buffer`: out = op(a, b, c)
  // with the per-limb constants, if any.  a, c wait for their producers (`from` empty: an op input, nothing to wait for); b is a stored operand
  Limbs eweStage(const std::string &key, ewe_opcode op, const std::string &buffer, const Limbs &a, const Limbs *c = nullptr,
                 const std::vector<uint64_t> &constants = {}, const std::vector<AddrType> &b = {});
  // the three polynomials d0, d1, d2 of a tensor product with their producers; its MAC2 records (d1) get the mark
  static std::array<Limbs, 3> tensorProduct(const TensorCompute &tcm, FusedForm mark);
  static std::array<std::vector<AddrType>, 3> addrs(const std::array<Limbs, 3> &d);
  // the same scalar on d0, d1, d2 (HSQUARE, HMULADD, HDOTADD): three MUL_CONST stages <key>_D<i> into <buffer>D<i>Scale<suffix>, constants `constants`
  void scaleTriple(std::array<Limbs, 3> &d, const std::string &key, const std::string &buffer, const std::string &suffix, const std::string &constants,
                   uint64_t stream);
  // the tail of HMULADD and HDOTADD on the running d: per addend t = 1..A (input ciphertext firstCt + t, stream + step t) and component k,
  // <op>_AddScale_(t)_C<k> (MUL_CONST, constants "addscale<t>") and <op>_Add_(t)_D<k> (ADD) into <buffer>D<k><sumWord>(t); shifted: <op>_Const_D0
  void addendTail(std::array<Limbs, 3> &d, const std::string &op, const std::string &buffer, const std::string &sumWord, uint32_t A, uint32_t firstCt,
                  uint64_t stream, uint64_t step, bool shifted, uint64_t constStream);
  // HLINCOMB's and HMLINCOMB's chain on component k: <op>_Scale_<index t)>_C<k> = s_t ct<t>.c<k> (MUL_CONST, stream + step t, constants <scale><t>;
  // term 1 carries the mark Lincomb), <op>_Add_<index t)>_C<k> for t >= 2, and with constHere <constKey>_C<k> (ADD_CONST, constants <constName>);
  // the last buffer is `result`
  struct ScaledSumNames { std::string op, index, result, constKey, scale, constName; uint64_t stream, step, constStream; };
  Limbs scaledSum(uint32_t k, uint32_t T, bool constHere, const ScaledSumNames &n);
  std::vector<AddrType> alloc(const std::string &name, uint32_t limbs);  // MallocMem + getAddr
  std::vector<AddrType> component(uint32_t ct, uint32_t k) const { return k == 0 ? cts[ct].getC0Addr() : cts[ct].getC1Addr(); }  // c_k of input ct
  void setOutput(const std::string &out, uint32_t k, const std::vector<AddrType> &limbs) { namedOutputs[out + ".c" + std::to_string(k)] = limbs; }
  void dispatch(const StageList &m);
  // the two halves of a rotation around its key switch, shared by HROTATE (suffix "") and HROTATE_HOISTED ("_Rot<r>"): sigma_g of component k
  // of ct1 into AUTOOutput<suffix>(k); and <out>.c0 = sigma_g(c0) + ks0, <out>.c1 = ks1
  Limbs rotateComponent(uint32_t k, uint32_t galois, const std::string &suffix, uint32_t ct = 0);   // ct: of input ciphertext ct<ct + 1>
  // ... of any `level` limbs (HBSGS: the c0 of an intermediate ciphertext), waiting for their producers `in.from` (empty: op inputs)
  Limbs rotateLimbs(const Limbs &in, uint32_t k, uint32_t galois, const std::string &suffix);
  void finishRotation(const std::string &out, const std::vector<AddrType> &rotatedC0, const KeySwitch::Output &ks, const std::string &suffix);
  void finishConstruction();  // registers every temporary with the backend
  // the chains of element-wise stages that the ops summing on the extended basis are built of (HLINTRANS, HROTSUM, HBSGS).  A sum is three buffers,
  // t = 0, 1: S_0, S_1 (tags Key0, Key1; the E = level + alpha limbs) and t = 2: U (tag C0; the `level` Q limbs); sumMods(t): their modulus ids.
  // With the identity step a fourth, t = 3: W (tag C1; the Q limbs), the unrotated c1 times the identity plaintext.
  struct SwitchedSum { Limbs c0; std::vector<AddrType> c1; };   // (U + ModDown(S_0), ModDown(S_1)); with the identity step W + ModDown(S_1)
  std::vector<uint32_t> sumMods(uint32_t t) const;
  // the weighted sum sum_r terms[r] * pts[r]: stages LinTrans_(<r>)_<tag><suffix>, buffers LinTransOut_temp(<r>)_<tag><suffix>, the last LinTransOut_<tag><suffix>
  // `head` / `headPt`: an unrotated head term in front of them (the identity step), rotation 0 in the names: the chain's MUL is then its
  Limbs weightedSum(uint32_t t, const std::vector<Limbs> &terms, const std::vector<std::vector<AddrType>> &pts, const std::string &suffix,
                    const Limbs *head = nullptr, const std::vector<AddrType> *headPt = nullptr);
  // the running sum: sum + term, the i-th term (i >= 2): stage and buffer <stem>_(<i>)_<tag>, the last buffer <stem>Out_<tag>
  Limbs addTerm(uint32_t t, const Limbs &sum, const Limbs &term, const std::string &stem, uint32_t i, bool last);
  // the tail: ModDown<suffix> of sums[0], sums[1], then c0 = its output 0 + sums[2] in stage <op>_Hadd<suffix>, buffer `buffer`
  // `c1Addend` (the identity step's W): c1 = the ModDown's output 1 + it in stage <op>_Hadd1<suffix>, buffer <op>Output<suffix>(1)
  SwitchedSum sumDown(KeySwitch &ks, const std::array<Limbs, 3> &sums, const std::string &op, const std::string &buffer, const std::string &suffix,
                      const Limbs *c1Addend = nullptr);
  void setOutput(const std::string &out, const SwitchedSum &ct, bool rescale = false);   // rescale: through setRescaledOutput

public:
  virtual ~OperationBase();
  bool simulate();   // upstream entry: banner, execute, stat block
  // backend = sim: run the cycle model to completion without the banner / progress output; false = no instruction retired
  // for 2000 cycles (upstream's dead-lock exit).  simulate() on the sim backend is this loop plus upstream's stdout.
  bool simulateCycles(bool verbose = false);
  void prepare();    // issue stages + allocate/fill/fuse (idempotent)
  double execute(uint32_t iters);  // ns per iteration of the whole op (device time)
  std::vector<AddrType> bufferAddrs(const std::string &name) const;  // named buffer (Malloc name, input or output alias)
  bool readBuffer(const std::string &name, uint64_t *host, uint32_t copy = 0);  // copy: op of the batch (config key `batch`)
  bool writeBuffer(const std::string &name, const uint64_t *host, uint32_t copy = 0);  // real data for an input / key buffer ([limbs][N], fully reduced)
  // fills the input plaintext `name` (pt of PMULT / PADD; pt<r>, pt0 of HLINTRANS / HBSGS; pt<t>, pt0 of HPLINCOMB) of op `copy` with the encoding
  // of N / 2 slots at scale `scale`: every limb the buffer has (level, or level + alpha on the extended basis) under its own modulus, encoded on
  // the device (hm_encode).  Prepares the op if needed; synchronises.  Refused with a message beginning "encode_plaintext:"
  // for an unknown name, a name that is no plaintext, a wrong length, backend != hip, world > 1, or a coefficient beyond half the largest modulus
  // (found after the encode: the buffer then holds the encoding with 0 in place of every such coefficient)
  void encodePlaintext(const std::string &name, const std::vector<std::complex<double>> &slots, double scale, uint32_t copy = 0);
  unsigned long long totalInstructions();
  // replaces the per-limb constants `name` of the op (HSQUARE: "scale", "const"; HLINCOMB: "scale1" .. "scale<T>", "const"; HMLINCOMB: "scale<m>_<t>", "const<m>"; HMULADD: "scale", "addscale1" .. "addscale<A>", "const"; HDOTADD: "scale1" .. "scale<T>", "addscale1" .. "addscale<A>", "const") by n = level residues, values[j] reduced mod q_j; before prepare() only.
  // Refused, by op and name: after prepare(), n != level, an unreduced value (or a zero where the constant multiplies), a name whose config key is 0
  void setConstants(const std::string &name, const uint64_t *values, uint32_t n);
  Arch *getArch() { return arch; }
  std::vector<std::string> bufferNames() const;
  // continuous execution: this op's input ciphertext `input` ("ct1", "ct2") is the output ciphertext `output` of `producer` ("out"; HREIM has a
  // second one, "out_im"); an output name the producer does not have is refused with the producer's op name
  void bindInput(const std::string &input, OperationBase *producer, const std::string &output = "out");
  uint32_t outputLevel() const;  // limbs of out.c0
  const std::string &name() const { return opName; }
};

class HMULT : public OperationBase {
public:
  HMULT(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
class HROTATE : public OperationBase {
public:
  HROTATE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hrotate_hoisted (build extension; the reference has no such op): R rotations of ONE ciphertext with ONE ModUp (config keys `rotations` = R,
// default 4, 1..16, and `galois` = g, default 5; rotation r = 1..R by g^r mod 2N).  Outputs out<r>.c0 / out<r>.c1, keys IP_Rot<r>_Key<k>_<j>.
class HROTATE_HOISTED : public OperationBase {
public:
  HROTATE_HOISTED(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hlintrans (build extension): sum_r pt_r (.) rot_r(ct1) over the R rotations of hrotate_hoisted (same config keys, same keys IP_Rot<r>_Key<k>_<j>),
// with ONE ModUp and ONE ModDown: the plaintexts pt<r> are given on the extended basis and the weighted sum is formed on it, before the ModDown.
// One output ciphertext out at the input's level; no rescale (as PMULT).
class HLINTRANS : public OperationBase {
public:
  HLINTRANS(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hdot (build extension): sum_t ct<2t-1> * ct<2t> over T pairs of ciphertexts (config key `terms` = T, default 4, 1..16) with ONE relinearisation
// and ONE rescale: the tensor products are summed first (d_i = sum_t d_i,t), then HMULT's tail runs once.  Inputs ct1 .. ct<2T>, key IP_Key<k>_<j>
// (hmult's), one output ciphertext out at level - 1.  Bit-identical to tensor + hadd of the d's + hmult's tail; terms = 1 is hmult.
class HDOT : public OperationBase {
public:
  HDOT(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hrotsum (build extension): sum_i rot_{g^i}(ct<i>) over G DIFFERENT ciphertexts (config keys rotations = G and galois = g as hrotate_hoisted, same
// keys IP_Rot<i>_Key<k>_<j>), with G ModUps and ONE ModDown: the key products are summed on the extended basis.  One output ciphertext out at the
// inputs' level; no rescale.
// hsquare (build extension): out = Rescale(Relin(s * ct1^2) + k), one double-angle step y <- 2 y^2 - 1 of EvalMod with s = 2, k = -Delta^2.  The tensor
// product of ct1 with ITSELF (d0 = a a, d1 = 2 a c, d2 = c c), then with config key sq_scale = 1 the per-limb scalars s_j on all three (synthetic:
// word 0 of limb j of stream seed + 6000, a 0 replaced by 1) and with sq_const = 1 the per-limb constants k_j on every evaluation-form entry of d0
// (stream seed + 6100), then HMULT's tail with hmult's key IP_Key<k>_<j>.  setConstants("scale" | "const") replaces the synthetic values.  One
// input, one output ciphertext out at level - 1.  With both keys 0 bit-identical to hmult of ct1 with itself.
class HSQUARE : public OperationBase {
public:
  HSQUARE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hlincomb (build extension): out = sum_t s_t * ct<t> + k, a linear combination of T ciphertexts at one level (config key terms = T as hdot: default 4,
// 1..16) with per-limb scalars s_{t,j} in [0, q_j) (synthetic: word 0 of limb j of stream seed + 6200 + 100 t; zero = the term contributes nothing)
// and, with config key lc_const = 1, per-limb constants k_j on every evaluation-form entry of c0 only (stream seed + 6290): the baby steps and the
// giant-step recombination of EvalMod's polynomial evaluation.  setConstants("scale<t>" | "const") replaces the synthetic values.  No key, no
// ModUp.  One output ciphertext out at the inputs' level, or through Rescale at level - 1 with config key rescale = 1.
class HLINCOMB : public OperationBase {
public:
  HLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hmlincomb (build extension): out<m> = sum_t s_{m,t} * ct<t> + k_m for m = 1..M, M linear combinations of the SAME T ciphertexts at one level
// (config keys terms = T as hlincomb: default 4, 1..16; outputs = M: default 4, 1..16) with per-limb scalars s_{m,t,j} in [0, q_j) (synthetic:
// word 0 of limb j of stream seed + 8000 + 1000 m + 100 + 50 t; zero = the term contributes nothing) and, with config key ml_const = 1, per-limb
// constants k_{m,j} on every evaluation-form entry of c0 only (stream seed + 8000 + 1000 m + 950): the baby blocks and the remainder of a
// Paterson-Stockmeyer evaluation, which are M combinations of the same baby powers.  setConstants("scale<m>_<t>" | "const<m>") replaces the
// synthetic values.  No key, no ModUp.  M output ciphertexts out1 .. out<M> at the inputs' level, or each through Rescale at level - 1 with
// config key rescale = 1; "out" names out1.  Bit-identical to M hlincomb ops with the same constants
class HMLINCOMB : public OperationBase {
public:
  HMLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hmuladd (build extension): out = Rescale(Relin(s * ct1 * ct2 + sum_t u_t * ct<2+t>) + k), one node of a polynomial evaluation (the Chebyshev step
// T_{a+b} = 2 T_a T_b - T_{|a-b|}, the Paterson-Stockmeyer recombination p = q T_g + r).  2 + A input ciphertexts at one level (config key addends = A,
// default 1, 0..8); with ma_scale = 1 the per-limb scalars s_j in [1, q_j) on the three polynomials of the tensor product (synthetic: word 0 of limb j
// of stream seed + 6400, a 0 replaced by 1); the addend scalars u_{t,j} in [0, q_j) (stream seed + 6400 + 10 t; zero = the addend contributes nothing);
// with ma_const = 1 the per-limb constants k_j on every evaluation-form entry of d0 only (stream seed + 6490).  All of it acts in front of the key
// switch, at scale Delta^2 on the level of the inputs; then HMULT's tail with hmult's key IP_Key<k>_<j>.  setConstants("scale" | "addscale<t>" |
// "const") replaces the synthetic values.  One output ciphertext out at level - 1.  A = 0 with both keys 0 is bit-identical to hmult.
class HMULADD : public OperationBase {
public:
  HMULADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hreim (build extension): the real and the imaginary part of the slots of ct1 with ONE key switch: conj = hrotate_{2N-1}(ct1), exactly as HROTATE
// computes it with hrotate's key IP_Key<k>_<j> (here the conjugation key; the config key galois is ignored), then per component
// out.c<k> = ct1.c<k> + conj.c<k> (slots 2 Re z) and out_im.c<k> = U (.) (ct1.c<k> - conj.c<k>) (slots 2 Im z), U the evaluation form of -X^(N/2),
// which the op keeps in its named buffer `unit` (level limbs, filled from the host's roots when the op is prepared: no input stream).  One input,
// two output ciphertexts out and out_im at the input's level; the conjugate itself is the named output conj.
class HREIM : public OperationBase {
public:
  HREIM(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hclincomb (build extension): out = sum_t (a_t + b_t X^(N/2)) * ct<t> + k, a complex-weighted sum of T ciphertexts at one level: on the slots X^(N/2) is
// the multiplication by i, so the weights are a_t + i b_t (config key terms = T as hlincomb: default 4, 1..16).  Per-limb scalars a_{t,j}, b_{t,j} in
// [0, q_j), either may be 0 (synthetic: word 0 of limb j of stream seed + 6450 + 100 t for a, seed + 8150 + 100 t for b) and, with config key
// cl_const = 1, per-limb real constants k_j on every evaluation-form entry of c0 only (stream seed + 9850): ct_re + i ct_im behind EvalMod, the
// product of a ciphertext by a Gaussian-integer constant, the recombination of a complex polynomial.  The op keeps U = -X^(N/2) in evaluation form in
// its named buffer `unit` as HREIM does.  setConstants("scale<t>" | "scale_im<t>" | "const") replaces the synthetic values ("scale_im<t>" takes b_t;
// the stage that multiplies by U stores its negation).  No key, no ModUp.  One output ciphertext out at the inputs' level, or through Rescale at
// level - 1 with config key rescale = 1.
class HCLINCOMB : public OperationBase {
public:
  HCLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hplincomb (build extension): out = (sum_t pt<t> (.) ct<t>.c0 + pt0, sum_t pt<t> (.) ct<t>.c1), a plaintext-weighted sum of T ciphertexts at one level
// (config key terms = T as hlincomb: default 4, 1..16).  pt<t> are named input plaintexts of `level` limbs in evaluation form on the ciphertext basis
// (synthetic: stream seed + 4000 + 100000 t, as hlintrans numbers its plaintexts; replaceable through writeBuffer("pt<t>", ...)); with config key
// pl_addend = 1 one more, pt0 (stream seed + 4000 + 100000 * 17), is added to c0 only, as PADD's plaintext: the inner sum of a baby-step/giant-step
// transform over rotations that already exist, masking and merging, a polynomial with slot-wise coefficients, a linear layer's bias.  No key, no
// ModUp.  One output ciphertext out at the inputs' level, or through Rescale at level - 1 with config key rescale = 1.
class HPLINCOMB : public OperationBase {
public:
  HPLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hdotadd (build extension): out = Rescale(Relin(sum_t s_t * ct<2t-1> * ct<2t> + sum_r u_r * ct<2T+r>) + k), one node of a polynomial evaluation with
// several products (the Paterson-Stockmeyer recombination p = sum_i q_i G_i + r, one component of a complex product).  2T + A input ciphertexts at
// one level >= 2 (config keys terms = T, default 4, 1..16, and addends = A, default 1, 0..8); with da_scale = 1 the per-pair per-limb scalars s_{t,j}
// in [1, q_j) on the three polynomials of pair t (synthetic: word 0 of limb j of stream seed + 6050 + 50 t, a 0 replaced by 1); the addend scalars
// u_{r,j} in [0, q_j) (stream seed + 7050 + 50 r; zero = the addend contributes nothing); with da_const = 1 the per-limb constants k_j on every
// evaluation-form entry of d0 only (stream seed + 7900).  All of it acts in front of the key switch, at scale Delta^2 on the level of the inputs;
// then HMULT's tail with hmult's key IP_Key<k>_<j>.  setConstants("scale<t>" | "addscale<r>" | "const") replaces the synthetic values.  One output
// ciphertext out at level - 1.  A = 0 with both keys 0 is bit-identical to hdot, T = 1 to hmuladd with the same constants.
class HDOTADD : public OperationBase {
public:
  HDOTADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
class HROTSUM : public OperationBase {
public:
  HROTSUM(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hbsgs (build extension): the baby-step/giant-step linear transform out = sum_i rot_{h^i}( sum_r pt<(i-1)R+r> (.) rot_{g^r}(ct1) ), i = 1..G (config
// key giants, default 4, 1..16; galois_giant = h, default g^R mod 2N), r = 1..R (rotations, galois as hlintrans, same keys IP_Rot<r>_Key<k>_<j>), with
// ONE ModUp of ct1 and one key product per baby rotation shared by the G inner sums; then hrotsum's body on the G intermediate ciphertexts with the
// keys IP_Giant<i>_Key<k>_<j>.  Bit-identical to G hlintrans ops + one hrotsum.  One output ciphertext out at the input's level; no rescale.
class HBSGS : public OperationBase {
public:
  HBSGS(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
class HADD : public OperationBase {
public:
  HADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
class PMULT : public OperationBase {
public:
  PMULT(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hrescale (build extension): out = Rescale of both components of ct1, at level - 1; the rescale of HMULT's tail as an op of its own, for what
// PMULT and the summing ops leave at scale Delta^2 (they take it themselves with rescale = 1)
class HRESCALE : public OperationBase {
public:
  HRESCALE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
// hmodraise (build extension): out = ModRaise of ct1 (level 1) to level T = config key raise_to (default maxLevel): every limb j < T of both
// components is NTT_{q_j} of the centred representative mod q_0 of the input's coefficients.  The one op whose output level is ABOVE its input's
class HMODRAISE : public OperationBase {
public:
  HMODRAISE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};
class PADD : public OperationBase {
public:
  PADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch);
};

// Continuous multi-op execution.  Upstream cannot chain operations ("NotSuppotr the continuous
// operation simulate", src/Operation.cpp:636): every op starts from freshly allocated inputs.  A chain keeps the
// ciphertext resident in HBM: op k+1's first input ciphertext IS op k's output (copied device to device,
// stream-ordered, no host round trip); its level follows the data (an hmult's rescale drops one limb).  Second
// operands (ct2 of hmult / hadd, the plaintext of pmult / padd) and the evaluation keys are synthetic as for single ops.
class OpChain {
  std::vector<Config *> cfgs;
  std::vector<Arch *> archs;
  std::vector<OperationBase *> ops;
public:
  // ops: comma-separated list of hmult | hrotate | hadd | pmult | padd | hlintrans | hdot | hrotsum | hbsgs | hrescale | hmodraise | hsquare | hlincomb | hmuladd | hreim | hclincomb | hplincomb | hdotadd | hmlincomb ("out" = its out1), e.g. "hmult,hrotate,hadd,hmult"; hrotate_hoisted (R output
  // ciphertexts) only as the last op
  OpChain(const std::string &cfgPath, const std::string &opList, uint32_t maxLevel, uint32_t curLevel, uint32_t alpha,
          const std::map<std::string, uint32_t> &overrides = {});
  ~OpChain();
  size_t size() const { return ops.size(); }
  OperationBase *op(size_t i) { return ops.at(i); }
  void prepare();
  void run();                        // one pass over the whole chain, asynchronous
  void sync();
  double execute(uint32_t iters);    // wall ns per pass over the chain (host clock around enqueue + sync)
  bool simulate();                   // CLI: per-op banners and stat blocks, then the chain total
};
#endif
