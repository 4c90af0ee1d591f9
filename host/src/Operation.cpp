// Operation.cpp — stage-graph builders.  Structure (stage keys, order, buffer names, limb counts) follows the
// reference's src/Operation.cpp, cited per function; the wiring is the mathematically correct one of
// SURVEY.md Appendix A (upstream only needs shapes, and mislabels several operands: Appendix C).
#include "Operation.h"
#include "SimProgram.h"
#include "../../include/homulator_hip.h"   // HM_TENSOR_MULADD_MAX_ADDENDS

#include <algorithm>
#include <cctype>
#include <chrono>
#include <numeric>
#include <sstream>

static std::string S(uint32_t v) { return std::to_string(v); }

// =====================================================================================================
// per-limb stages
// =====================================================================================================
// "n limbs, one instruction each": instruction i, named pre + i + post, works at level firstLevel + i under modulus mods[i] (n = mods.size())
// and writes out[i] from the operand lists that are set.  A list left empty is an absent operand (address 0, InsGen.h); a list of one address
// serves every limb.  `after` = the stages whose limb-i group the instruction depends on, in the order of its dependency list (a stage of one
// group: every limb depends on it).  constants: the per-limb constant of MUL_CONST / SUB_SCALE; empty = none.
struct PerLimb {
  std::string pre, post;
  std::vector<uint32_t> mods;
  std::vector<AddrType> out, a, b, c, d;
  std::vector<const std::vector<INSGROUP> *> after;
  std::vector<uint64_t> constants;
  uint32_t firstLevel = 0;

  template <class T> static const T &pick(const std::vector<T> &v, uint32_t i) { return v.at(v.size() == 1 ? 0 : i); }
  AddrType operand(const std::vector<AddrType> &v, uint32_t i) const { return v.empty() ? 0 : pick(v, i); }
  // the generators only read their dependency groups
  INSGROUP *dep(size_t k, uint32_t i) const { return k < after.size() ? const_cast<INSGROUP *>(&pick(*after[k], i)) : nullptr; }
  std::string name(uint32_t i) const { return pre + S(i) + post; }
};
// one InsGen::GenEWE per limb
static std::vector<INSGROUP> eweLimbs(InsGen *gen, ewe_opcode opcode, const PerLimb &s) {
  std::vector<INSGROUP> g;
  for (uint32_t i = 0; i < s.mods.size(); i++)
    g.push_back(gen->GenEWE(s.firstLevel + i, s.name(i), s.dep(0, i), s.dep(1, i), s.dep(2, i), s.dep(3, i), s.operand(s.a, i), s.operand(s.b, i),
                            s.operand(s.c, i), s.operand(s.d, i), s.out.at(i), opcode, s.mods[i], !s.constants.empty(),
                            s.constants.empty() ? 0 : s.constants.at(i)));
  return g;
}
// one InsGen::GenNTT per limb, forward or inverse transform of a: one operand, at most one stage to wait for
static std::vector<INSGROUP> nttLimbs(InsGen *gen, bool forward, const PerLimb &s) {
  std::vector<INSGROUP> g;
  for (uint32_t i = 0; i < s.mods.size(); i++)
    g.push_back(gen->GenNTT(s.firstLevel + i, s.name(i), s.dep(0, i), forward, s.operand(s.a, i), s.out.at(i), s.mods[i]));
  return g;
}
// one InsGen::GenAUTO per limb (src/InsGen.cpp:46-71): sigma_galois of a
static std::vector<INSGROUP> autoLimbs(InsGen *gen, uint32_t galois, const PerLimb &s) {
  std::vector<INSGROUP> g;
  for (uint32_t i = 0; i < s.mods.size(); i++)
    g.push_back(gen->GenAUTO(s.firstLevel + i, s.name(i), s.dep(0, i), s.operand(s.a, i), s.out.at(i), galois, s.mods[i]));
  return g;
}

static std::vector<uint32_t> range(uint32_t lo, uint32_t n) {
  std::vector<uint32_t> v(n);
  std::iota(v.begin(), v.end(), lo);
  return v;
}
template <class T> static std::vector<T> slice(const std::vector<T> &v, uint32_t lo, uint32_t n) { return std::vector<T>(v.begin() + lo, v.begin() + lo + n); }
static Limbs slice(const Limbs &b, uint32_t lo, uint32_t n) { return {slice(b.addr, lo, n), slice(b.from, lo, n)}; }
static std::vector<AddrType> alloc(AddrManage *mem, const std::string &name, uint32_t limbs) {
  mem->MallocMem(name, limbs);
  return mem->getAddr(name);
}
static AddrType allocTable(AddrManage *mem, const std::string &name) {  // a base-conversion table: an address token (InsGen.h)
  mem->MallocMemOneBatch(name, 1);
  return mem->getAddr(name)[0];
}
static uint64_t invMod(uint64_t a, uint64_t q) {  // a^-1 mod q by Fermat
  uint64_t base = a % q, e = q - 2, r = 1;
  for (; e; e >>= 1) {
    if (e & 1) r = (uint64_t)(((unsigned __int128)r * base) % q);
    base = (uint64_t)(((unsigned __int128)base * base) % q);
  }
  return r;
}

// =====================================================================================================
// KeySwitch — reference: KeySwitch::KeySwitch src/Operation.cpp:9-54 (stage order), beta = ceil(l/alpha) :22
// =====================================================================================================
// same signature as upstream (include/Operation.h:48-54): the backend and the key seed travel with the generator
KeySwitch::KeySwitch(std::string labelName, uint32_t maxlevel, uint32_t level, uint32_t alpha, std::vector<AddrType> *,
                     std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen, AddrManage *memoryMange)
    : DataInsMap(map), insGenPointer(insgen), Level(level), Alpha(alpha), Beta((level + alpha - 1) / alpha), MaxLevel(maxlevel),
      memMange(memoryMange), arch(insgen->backend()), baseName(labelName + "_KeySwitch"), qMods(range(0, level)), pMods(range(maxlevel, alpha)),
      extMods(qMods) {
  extMods.insert(extMods.end(), pMods.begin(), pMods.end());  // extended limb order = Q limbs then P limbs: Appendix A (3)
}

KeySwitch::KeySwitch(std::string labelName, uint32_t maxlevel, uint32_t level, uint32_t alpha,
                     const std::vector<AddrType> &inputPolynomialAddress, std::vector<AddrType> *pool,
                     std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen, AddrManage *memoryMange)
    : KeySwitch(labelName, maxlevel, level, alpha, pool, map, insgen, memoryMange) {
  out_ = modDown(keyProduct(modUp(inputPolynomialAddress, false), insgen->keySeed(), ""), "");
}

// reference: KeySwitch::KeySwitch :33-40 — the ModUp: INTT of the input, then per digit scale, conversion and forward transforms
KeySwitch::Digits KeySwitch::modUp(const std::vector<AddrType> &input, bool inputMayBeOpInput, const std::string &suffix) {
  const std::string baseName = this->baseName + suffix;
  const uint32_t E = Level + Alpha;
  // reference: KeySwitch::ModUpINTT :63-102 — one INTT per input limb; throws when the input has no producer, unless it may be the op's own input
  // ciphertext (the hoisted rotations)
  PerLimb in{baseName + "_ModUp_INTT(", ")_", qMods, alloc(memMange, "ModUpINTTOut" + suffix, Level)};
  std::vector<INSGROUP> producers;
  for (uint32_t l = 0; l < Level; l++) {
    auto prod = DataInsMap->find(input[l]);
    if (prod == DataInsMap->end() && !inputMayBeOpInput) throw std::runtime_error("Error! This dependece need exists!\n\n");
    producers.push_back(prod == DataInsMap->end() ? INSGROUP() : prod->second);
  }
  in.a = input;
  in.after = {&producers};
  const Limbs intt{in.out, stages.add("ModUp_INTT" + suffix, nttLimbs(insGenPointer, false, in))};
  const std::vector<AddrType> offset = alloc(memMange, "ModUpDecompOffset" + suffix, 1), decompOut = alloc(memMange, "ModUpDecompOut" + suffix, Level);

  Digits digits;
  for (uint32_t be = 0; be < Beta; be++) {
    const uint32_t lo = be * Alpha, dj = std::min(Alpha, Level - lo);
    const std::string B = S(be), B_ = suffix + "_(" + B + ")";
    // reference: ModUpDecompFusionBConvStep1 :104-135 — y_i = x_i * [(Q_Dj/q_i)^-1]_{q_i} for the limbs of digit j
    const Limbs x = slice(intt, lo, dj);
    PerLimb sc{baseName + "_decompFusionBConvStep1_beta(" + B + ")_Level(", ")_", range(lo, dj), slice(decompOut, lo, dj)};
    sc.firstLevel = lo;
    sc.a = x.addr;
    sc.b = offset;
    sc.after = {&x.from};
    sc.constants = arch->bconvScale(sc.mods);
    std::vector<INSGROUP> &scaled = stages.add("ModUp_DecompOut" + suffix + B + ")", eweLimbs(insGenPointer, EWE_MUL_CONST, sc));  // sic: upstream's key has the stray parenthesis (:133)

    // reference: ModUpBConvStep2 :137-188 — every limb of the extended basis outside the digit, d_j-deep MAC each
    // reference: ModUpNTT :190-292 — E NTT instructions per digit.  Upstream also spends an NTT on each of the
    // digit's own limbs; mathematically those are the original evaluation-form input limbs, so here they are
    // pass-through records (a copy, or nothing once the consumers are redirected) that still count as NTTs.
    const AddrType table = allocTable(memMange, "BConvMap" + B_);
    const std::vector<AddrType> convOut = alloc(memMange, "BConvOut" + B_, E - dj), digit = alloc(memMange, "NTTOut" + suffix + "_beta(" + B + ")", E);
    std::vector<INSGROUP> conv, ntt;
    for (uint32_t t = 0; t < E; t++) {
      const std::string name = baseName + "_ModUp_NTT_beta(" + B + ")_Level(" + S(t) + ")_";
      if (t >= lo && t < lo + dj) {
        ntt.push_back(insGenPointer->GenNTT(t, name, &scaled[t - lo], true, input[t], digit[t], t, /*passthrough=*/true));
      } else {
        const uint32_t o = (uint32_t)conv.size();
        conv.push_back(insGenPointer->GenBCONV(o, dj, baseName + "_ModUpBConv_beta(" + B + ")_outLevel(" + S(t) + ")_", scaled, sc.out, sc.mods, table,
                                               convOut[o], extMods[t]));
        ntt.push_back(insGenPointer->GenNTT(t, name, &conv[o], true, convOut[o], digit[t], extMods[t]));
      }
    }
    stages.add("ModUp_BCONV" + B_, conv);
    digits.push_back({digit, stages.add("ModUp_NTT" + B_, ntt)});
  }
  return digits;
}

// hoisted rotations: sigma_g of every extended digit of the shared ModUp, one AUTO per limb, into AUTOOut<suffix>_beta(j): what the key product of
// this rotation reads instead of the digits themselves
KeySwitch::Digits KeySwitch::rotateDigits(const Digits &digits, uint32_t galois, const std::string &suffix) {
  Digits rotated;
  for (uint32_t j = 0; j < digits.size(); j++) {
    const std::string J = S(j);
    PerLimb s{baseName + suffix + "_AUTO_beta(" + J + ")_Level(", ")_", extMods, alloc(memMange, "AUTOOut" + suffix + "_beta(" + J + ")", Level + Alpha)};
    s.a = digits[j].addr;
    s.after = {&digits[j].from};
    rotated.push_back({s.out, stages.add("AUTO" + suffix + "_beta(" + J + ")", autoLimbs(insGenPointer, galois, s))});
  }
  return rotated;
}

// reference: InnerProduceOperation :294-414 — acc_k = sum_j ext_j * evk_{j,k}; beta = 1: one product (:314-352);
// beta > 1: beta-1 MAC groups, the first with two products (:355-411).  The last group writes
// InnerProduceOut_Key<k> (upstream writes a temp and reads a buffer nobody produced: Appendix C item 3).
KeySwitch::Accumulators KeySwitch::keyProduct(const Digits &x, uint64_t keySeed, const std::string &suffix) {
  const uint32_t E = Level + Alpha, groups = Beta == 1 ? 1 : Beta - 1;
  Accumulators acc;
  for (uint32_t k = 0; k < 2; k++) {
    const std::string K = S(k);
    acc[k].addr = alloc(memMange, "InnerProduceOut" + suffix + "_Key" + K, E);
    std::vector<std::vector<AddrType>> key, temp;
    for (uint32_t be = 0; be < Beta; be++) {
      key.push_back(alloc(memMange, "IP" + suffix + "_Key" + K + "_" + S(be), E));
      // evaluation key limbs are inputs: deterministic synthetic stream (same layout as the oracle's synth_evk)
      arch->addInputFill(InputFill{key[be], extMods, keySeed + (be * 2 + k) * 1000ull, /*shared=*/true});
      if (be + 2 <= Beta) temp.push_back(alloc(memMange, "InnerProduceOut" + suffix + "_temp(" + S(be) + ")_Key" + K, E));
    }
    const std::vector<INSGROUP> *sum = nullptr;  // the latest group
    for (uint32_t g = 0; g < groups; g++) {
      PerLimb s{baseName + suffix + "_InnerProducOperation(" + S(g) + ")_Level(", ")_Key(" + K + ")", extMods, g + 2 < Beta ? temp[g] : acc[k].addr};
      if (g == 0) {  // x_0 evk_0 [+ x_1 evk_1]
        s.a = x[0].addr;
        s.b = key[0];
        s.after = {&x[0].from};
        if (Beta > 1) {
          s.c = x[1].addr;
          s.d = key[1];
          s.after.push_back(&x[1].from);
        }
      } else {  // x_{g+1} evk_{g+1} + the group before
        s.a = x[g + 1].addr;
        s.b = key[g + 1];
        s.c = temp[g - 1];
        s.after = {&x[g + 1].from, sum};
      }
      sum = &stages.add("InnerProOut" + suffix + "_(" + S(g) + ")_Key" + K, eweLimbs(insGenPointer, Beta == 1 ? EWE_MUL : g == 0 ? EWE_MAC2 : EWE_MAC_ADD, s));
    }
    acc[k].from = *sum;
  }
  return acc;
}

// the ModDown of both accumulators, stage by stage (reference: KeySwitch::KeySwitch :46-53)
KeySwitch::Output KeySwitch::modDown(const Accumulators &acc, const std::string &suffix) {
  const std::string base = baseName + suffix;
  auto perKey = [&](const char *family, uint32_t k) { return family + suffix + "_Key(" + S(k) + ")"; };
  auto post = [](uint32_t k) { return ")_Key(" + S(k) + ")"; };
  std::array<Limbs, 2> intt, scaled, conv, ntt;
  Output out;
  // reference: ModDownINTT :417-445 — INTT of the alpha special-prime limbs of each inner-product output
  for (uint32_t k = 0; k < 2; k++) {
    const Limbs p = slice(acc[k], Level, Alpha);
    PerLimb s{base + "_ModDown_INTT(", post(k), pMods, alloc(memMange, perKey("INTTOut_ModDown", k), Alpha)};
    s.a = p.addr;
    s.after = {&p.from};
    intt[k] = {s.out, stages.add(perKey("ModDownINTTOut", k), nttLimbs(insGenPointer, false, s))};
  }
  // reference: ModDownBConvStep1 :447-487 — y_p = a_p * [(P/p)^-1]_p
  const std::vector<AddrType> ref = alloc(memMange, "ModDownBConvStep1" + suffix + "_Ref", 2);
  const std::vector<uint64_t> phatInv = arch->bconvScale(pMods);
  for (uint32_t k = 0; k < 2; k++) {
    const std::string name = perKey("ModDownBConvStep1", k);  // the buffer and the stage key
    PerLimb s{base + "_ModDownBConvStep1_Level(", post(k), pMods, alloc(memMange, name, Alpha)};
    s.a = intt[k].addr;
    s.b = {ref[k]};
    s.after = {&intt[k].from};
    s.constants = phatInv;
    scaled[k] = {s.out, stages.add(name, eweLimbs(insGenPointer, EWE_MUL_CONST, s))};
  }
  // reference: ModDownBConvStep2 :489-519 — P -> Q conversion, alpha inputs per output limb
  const AddrType table = allocTable(memMange, "ModdownBConvMap" + suffix);
  for (uint32_t k = 0; k < 2; k++) {
    conv[k].addr = alloc(memMange, "ModdownBConvOut" + suffix + "_Key" + S(k), Level);
    for (uint32_t ol = 0; ol < Level; ol++)
      conv[k].from.push_back(insGenPointer->GenBCONV(ol, Alpha, base + "_ModDownBConv_outLevel(" + S(ol) + post(k), scaled[k].from, scaled[k].addr, pMods,
                                                     table, conv[k].addr[ol], ol));
    stages.add(perKey("ModDown_BCONV", k), conv[k].from);
  }
  // reference: ModDowNTT :521-546 (passes ntt=false there: a labelling slip, Appendix C item 5)
  for (uint32_t k = 0; k < 2; k++) {
    PerLimb s{base + "_ModDown_NTT(", post(k), qMods, alloc(memMange, perKey("NTTOut_ModDown", k), Level)};
    s.a = conv[k].addr;
    s.after = {&conv[k].from};
    ntt[k] = {s.out, stages.add(perKey("ModDownNTTOut", k), nttLimbs(insGenPointer, true, s))};
  }
  // reference: ModDownSub :548-590 — ks_k,i = (acc_k,i - w_k,i) * [P^-1]_{q_i}
  std::vector<uint64_t> pInv;
  for (uint32_t l = 0; l < Level; l++) {
    const uint64_t q = arch->modulus(l);
    unsigned __int128 P = 1;
    for (uint32_t p : pMods) P = (P * (arch->modulus(p) % q)) % q;
    pInv.push_back(invMod((uint64_t)P, q));
  }
  for (uint32_t k = 0; k < 2; k++) {
    const std::string name = perKey("KeySwitchFinalOutput", k);  // the buffer and the stage key
    PerLimb s{base + "_ModDownSub_Level(", post(k), qMods, alloc(memMange, name, Level)};
    s.a = acc[k].addr;
    s.c = ntt[k].addr;
    s.after = {&ntt[k].from, &acc[k].from};
    s.constants = pInv;
    stages.add(name, eweLimbs(insGenPointer, EWE_SUB_SCALE, s));
    out[k] = s.out;
  }
  return out;
}

// =====================================================================================================
// TensorCompute — reference: src/Operation.cpp:592-739 (d0 = c00*c10, d1 = c00*c11 + c01*c10, d2 = c01*c11)
// =====================================================================================================
TensorCompute::TensorCompute(std::string labelName, uint32_t level, Ciphertext *cipher1, Ciphertext *cipher2,
                             std::vector<AddrType> *, std::map<AddrType, std::vector<Instruction *>> *, InsGen *insgen,
                             AddrManage *memoryMange, const std::string &bufferPrefix, const std::string &bufferSuffix) {
  const std::vector<AddrType> c00 = cipher1->getC0Addr(), c01 = cipher1->getC1Addr(), c10 = cipher2->getC0Addr(), c11 = cipher2->getC1Addr();
  auto buffer = [&](const char *d) { return bufferPrefix + d + "Out" + bufferSuffix; };
  PerLimb d0{labelName + "_TensorCompute_D0_Level(", ")", range(0, level), alloc(memoryMange, buffer("D0"), level)};  // computeD0 :624-660
  d0.a = c00;
  d0.b = c10;
  stages.add("TensorCompute_INS_D0", eweLimbs(insgen, EWE_MUL, d0));
  PerLimb d1{labelName + "_TensorCompute_D1_Level(", ")", d0.mods, alloc(memoryMange, buffer("D1"), level)};  // computeD1 :662-699
  d1.a = c00;
  d1.b = c11;
  d1.c = c01;
  d1.d = c10;
  stages.add("TensorCompute_INS_D1", eweLimbs(insgen, EWE_MAC2, d1));
  PerLimb d2{labelName + "_TensorCompute_D2_Level(", ")", d0.mods, alloc(memoryMange, buffer("D2"), level)};  // computeD2 :701-739
  d2.a = c01;
  d2.b = c11;
  stages.add("TensorCompute_INS_D2", eweLimbs(insgen, EWE_MUL, d2));
  d_ = {d0.out, d1.out, d2.out};
}

// =====================================================================================================
// Rescale — reference: src/Operation.cpp:741-911.  r = INTT_{q_last}(x_last);
// x'_i = (x_i - NTT_{q_i}(r)) * [q_last^-1]_{q_i}.  Upstream issues ONE forward NTT per polynomial (:810-822);
// the maths needs one per remaining limb.  The extra NTTs are emitted with refInstructions = 0 so that the
// instruction total still equals upstream's, and write into <base>_Rescale_Mul_Offset (a constants token
// upstream; same buffer list, every stage writes its own buffer).
// =====================================================================================================
Rescale::Rescale(std::string labelName, uint32_t level, const std::vector<AddrType> &input, std::vector<AddrType> *,
                 std::map<AddrType, std::vector<Instruction *>> *map, InsGen *insgen, AddrManage *mem, bool inputMayBeOpInput) {
  Arch *arch = insgen->backend();  // upstream's signature (include/Operation.h:156-162)
  const std::string base = labelName + "_Rescale";
  if (level < 2) throw std::runtime_error("Rescale needs at least two limbs");
  const uint32_t last = level - 1;
  // NTTOps :766-825.  All five buffers up front, in upstream's allocation order (:768-769, :828, :881-882)
  const std::vector<AddrType> r = alloc(mem, base + "_ResINTTOut", 1);
  alloc(mem, base + "_ResNTTOut", 1);
  const std::vector<AddrType> subOut = alloc(mem, base + "_Rescale_SubOut", last);
  out_ = alloc(mem, base + "_Rescale_MulOut", last);
  const std::vector<AddrType> nttOut = alloc(mem, base + "_Rescale_Mul_Offset", last);
  // throws when the last limb has no producer, unless the input may be the op's own input ciphertext (HRESCALE), as KeySwitch::modUp
  auto prod = map->find(input[last]);
  if (prod == map->end() && !inputMayBeOpInput) throw std::runtime_error("Error! This dependece need exists!\n\n");
  INSGROUP producer = prod == map->end() ? INSGROUP() : prod->second;
  const std::vector<INSGROUP> &intt =
      stages.add("Rescale_INTT", {insgen->GenNTT(0, base + "_Rescale_INTT(0)_", &producer, false, input[last], r[0], last)});

  const uint64_t qlast = arch->modulus(last);
  std::vector<uint64_t> qlastInv;
  for (uint32_t l = 0; l < last; l++) {
    // the forward transform accepts inputs below 4 q_l (lazy butterflies), so r in [0, q_last) needs no
    // separate reduction mod q_l as long as q_last < 4 q_l — true for any chain of same-size primes
    if (qlast >= 4 * arch->modulus(l)) throw std::runtime_error("Rescale: q_last >= 4 q_l is not supported");
    qlastInv.push_back(invMod(qlast, arch->modulus(l)));
  }
  PerLimb n{base + "_Rescale_NTT_level(", ")", range(0, last), nttOut};
  n.a = r;
  n.after = {&intt};
  const std::vector<INSGROUP> &ntt = stages.add("Rescale_NTT", nttLimbs(insgen, true, n));
  for (uint32_t l = 1; l < last; l++) ntt[l][0]->refInstructions = 0;

  PerLimb s{base + "_Rescale_Sub_Level(", ")", n.mods, subOut};  // SubOps :827-875
  s.a = input;
  s.c = nttOut;
  s.after = {&ntt};
  const std::vector<INSGROUP> &sub = stages.add("Rescale_SUB", eweLimbs(insgen, EWE_SUB, s));

  PerLimb m{base + "_Rescale_Mul_Level(", ")", n.mods, out_};  // MulOps :877-910
  m.a = subOut;
  m.b = nttOut;
  m.after = {&sub};
  m.constants = qlastInv;
  stages.add("Rescale_Mul", eweLimbs(insgen, EWE_MUL_CONST, m));
}

// =====================================================================================================
// OperationBase
// =====================================================================================================
OperationBase::OperationBase(const std::string &op, const std::string &labelName, Config *cfg, Arch *_arch, uint32_t maxLevel, uint32_t curLevel,
                             uint32_t alpha)
    : insgener(cfg), driver(cfg), arch(_arch), config(cfg), opName(op), label(labelName), maxLevel_(maxLevel), level_(curLevel), alpha_(alpha) {
  batchSize = cfg->getValue("batchSize");
  N = cfg->getValue("N");
  seed = cfg->getValueOr("seed", 0x484F4D55u);
  insgener.setGlobalDatapPoll(&Datapool);
  insgener.setGlobalDataInsMap(&DataInsMap);
  insgener.setBackend(arch);
  insgener.setKeySeed(seed + 10000);
  arch->bindParams(maxLevel, curLevel, alpha);
  Datapool.push_back(BASEADDRESS);
}
OperationBase::~OperationBase() {
  for (auto &kv : DataInsMap)
    for (Instruction *i : kv.second) delete i;
}
void OperationBase::makeInputs(uint32_t ciphertexts, bool plaintext, uint32_t extPlaintexts, const NamedStreams &namedExt, const NamedStreams &namedLevel) {
  for (uint32_t i = 0; i < ciphertexts; i++) {
    cts.emplace_back(level_, N, Datapool, batchSize);
    const std::vector<AddrType> c0 = cts[i].getC0Addr(), c1 = cts[i].getC1Addr();
    const std::string name = "ct" + S(i + 1);
    arch->registerLimbs(c0);
    arch->registerLimbs(c1);
    arch->addInputFill(InputFill{c0, range(0, level_), seed + 2000 * i});
    arch->addInputFill(InputFill{c1, range(0, level_), seed + 2000 * i + 1000});
    namedInputs[name + ".c0"] = c0;
    namedInputs[name + ".c1"] = c1;
  }
  if (plaintext) {
    ptx.reset(new Plaintext(level_, N, Datapool, batchSize));
    arch->registerLimbs(ptx->getC0Addr());
    arch->addInputFill(InputFill{ptx->getC0Addr(), range(0, level_), seed + 4000});
    namedInputs["pt"] = ptx->getC0Addr();
    plaintextMods["pt"] = range(0, level_);
  }
  std::vector<uint32_t> extMods = range(0, level_);
  for (uint32_t p : range(maxLevel_, alpha_)) extMods.push_back(p);
  for (uint32_t r = 1; r <= extPlaintexts; r++) {
    extPtx.emplace_back(level_ + alpha_, N, Datapool, batchSize);
    const std::vector<AddrType> pt = extPtx.back().getC0Addr();
    arch->registerLimbs(pt);
    arch->addInputFill(InputFill{pt, extMods, seed + 4000 + 100000ull * r});
    namedInputs["pt" + S(r)] = pt;
    plaintextMods["pt" + S(r)] = extMods;
  }
  for (const auto &ns : namedExt) {   // behind the numbered ones: an op without them keeps its address plan
    extPtx.emplace_back(level_ + alpha_, N, Datapool, batchSize);
    const std::vector<AddrType> pt = extPtx.back().getC0Addr();
    arch->registerLimbs(pt);
    arch->addInputFill(InputFill{pt, extMods, seed + ns.second});
    namedInputs[ns.first] = pt;
    plaintextMods[ns.first] = extMods;
  }
  for (const auto &ns : namedLevel) {   // behind everything else: an op without them keeps its address plan
    levelPtx.emplace_back(level_, N, Datapool, batchSize);
    const std::vector<AddrType> pt = levelPtx.back().getC0Addr();
    arch->registerLimbs(pt);
    arch->addInputFill(InputFill{pt, range(0, level_), seed + ns.second});
    namedInputs[ns.first] = pt;
    plaintextMods[ns.first] = range(0, level_);
  }
  addrManager.reset(new AddrManage(Datapool.back() + 1, batchSize));
  addrManager->setGlobalDatapPoll(&Datapool);
}
std::vector<AddrType> OperationBase::alloc(const std::string &name, uint32_t limbs) { return ::alloc(addrManager.get(), name, limbs); }
void OperationBase::dispatch(const StageList &m) {
  for (const auto &stage : m) driver.dispatchInstructions(stage.first, stage.second);
}
Limbs OperationBase::rotateComponent(uint32_t k, uint32_t galois, const std::string &suffix, uint32_t ct) {
  return rotateLimbs(Limbs{component(ct, k), {}}, k, galois, suffix);
}
Limbs OperationBase::rotateLimbs(const Limbs &in, uint32_t k, uint32_t galois, const std::string &suffix) {
  PerLimb s{label + "_AUTO" + suffix + "_Level(", ")_k(" + S(k) + ")", range(0, level_), alloc("AUTOOutput" + suffix + "(" + S(k) + ")", level_)};
  s.a = in.addr;
  if (!in.from.empty()) s.after = {&in.from};
  const Limbs rotated{s.out, autoLimbs(&insgener, galois, s)};
  driver.dispatchInstructions("AUTO" + suffix + "_Key(" + S(k) + ")", rotated.from);
  return rotated;
}
std::vector<uint32_t> OperationBase::hoistedRotations(const std::string &op) const {
  if (arch->backend() == Arch::BACKEND_SIM) throw std::runtime_error(op + ": backend = sim has no such op (the reference has no hoisted rotation)");
  if (arch->world() > 1) throw std::runtime_error(op + ": world > 1 is not supported (sharded hoisting is not built)");
  const uint32_t R = config->getValueOr("rotations", 4), galois = config->getValueOr("galois", 5), twoN = 2 * N;
  if (R < 1 || R > 16) throw std::runtime_error(op + ": rotations = " + S(R) + ", must be in [1, 16]");
  if (!(galois & 1) || galois >= twoN) throw std::runtime_error(op + ": galois = " + S(galois) + " must be odd and below 2N = " + S(twoN));
  std::vector<uint32_t> gs;
  uint64_t gr = 1;
  for (uint32_t r = 1; r <= R; ++r) {
    gr = gr * galois % twoN;
    if (gr == 1 || std::find(gs.begin(), gs.end(), (uint32_t)gr) != gs.end())
      throw std::runtime_error(op + ": galois^" + S(r) + " mod 2N repeats an element or is 1: the " + S(R) + " rotations are not distinct");
    gs.push_back((uint32_t)gr);
  }
  return gs;
}
bool OperationBase::identityStep(const std::string &op) const {
  const uint32_t id = config->getValueOr("identity", 0);
  if (id > 1) throw std::runtime_error(op + ": identity = " + S(id) + ", must be 0 or 1");
  return id == 1;
}
bool OperationBase::rescaleKey(const std::string &op) const {
  const uint32_t rs = config->getValueOr("rescale", 0);
  if (rs > 1) throw std::runtime_error(op + ": rescale = " + S(rs) + ", must be 0 or 1");
  return rs == 1;
}
void OperationBase::setRescaledOutput(const std::string &out, const std::array<std::vector<AddrType>, 2> &ct, bool inputMayBeOpInput) {
  for (uint32_t k = 0; k < 2; k++) {
    Rescale res(label + "_" + S(k), level_, ct[k], &Datapool, &DataInsMap, &insgener, addrManager.get(), inputMayBeOpInput);
    dispatch(res.getInsMap());
    setOutput(out, k, res.output());
  }
}
// reference: HMULT::HMULT :947-1023, behind the tensor product
void OperationBase::relinearizeAndRescale(const std::array<std::vector<AddrType>, 3> &d) {
  KeySwitch ksw(label, maxLevel_, level_, alpha_, d[2], &Datapool, &DataInsMap, &insgener, addrManager.get());
  dispatch(ksw.getInsMap());
  std::array<std::vector<AddrType>, 2> sum;
  for (uint32_t k = 0; k < 2; k++) {
    PerLimb s{label + "_HMULTHadd_Level(", ")_k(" + S(k) + ")", range(0, level_), alloc("HMULTHaddOutput(" + S(k) + ")", level_)};
    s.a = ksw.output()[k];
    s.c = d[k];
    driver.dispatchInstructions("HMULT_Hadd_Key(" + S(k) + ")", eweLimbs(&insgener, EWE_ADD, s));
    sum[k] = s.out;
  }
  for (uint32_t k = 0; k < 2; k++) {
    Rescale res(label + "_" + S(k), level_, sum[k], &Datapool, &DataInsMap, &insgener, addrManager.get());
    dispatch(res.getInsMap());
    setOutput("out", k, res.output());
  }
}
void OperationBase::setConstants(const std::string &name, const uint64_t *values, uint32_t n) {
  std::string op = opName;
  std::transform(op.begin(), op.end(), op.begin(), [](unsigned char ch) { return (char)std::tolower(ch); });
  const std::string what = op + ": set_constants(\"" + name + "\")";
  auto cs = constantStages.find(name);
  if (cs == constantStages.end()) throw std::runtime_error(what + ": the op has no constants of that name");
  if (!cs->second.enabled) throw std::runtime_error(what + ": " + cs->second.key + " = 0, the op carries no such constants");
  if (arch->isPrepared()) throw std::runtime_error(what + " after prepare(): the plan is built");
  if (!values) throw std::runtime_error(what + ": null values");
  if (n != level_) throw std::runtime_error(what + ": n = " + S(n) + " values, the level is " + S(level_));
  for (uint32_t j = 0; j < n; ++j) {
    if (values[j] >= arch->modulus(j)) throw std::runtime_error(what + ": values[" + S(j) + "] is not reduced mod q_" + S(j));
    if (cs->second.nonZero && values[j] == 0) throw std::runtime_error(what + ": values[" + S(j) + "] is zero");
  }
  for (uint32_t j = 0; j < n; ++j)
    for (Instruction *i : cs->second.records[j]) i->constant = cs->second.negated && values[j] ? arch->modulus(j) - values[j] : values[j];
}
static uint64_t synthWord0(uint64_t stream, uint64_t q) {   // word 0 of a limb of the synthetic stream (hm_synth / ho_fill_uniform at x = 0)
  uint64_t z = stream * 0xD1342543DE82EF95ull + 0x632BE59BD9B4E019ull;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint64_t)(((unsigned __int128)z * q) >> 64);
}
// ---- what the builders of the fused element-wise ops share (HREIM, HDOT .. HDOTADD)
void OperationBase::refuseSimAndSharded(const std::string &op, const std::string &why) const {
  if (arch->backend() == Arch::BACKEND_SIM) throw std::runtime_error(op + ": backend = sim has no such op (" + why + ")");
  if (arch->world() > 1) throw std::runtime_error(op + ": world > 1 is not supported (the sharded plan is not built)");
}
bool OperationBase::flag(const std::string &op, const char *key, uint32_t dflt) const {
  const uint32_t v = config->getValueOr(key, dflt);
  if (v > 1) throw std::runtime_error(op + ": " + key + " = " + S(v) + ", must be 0 or 1");
  return v == 1;
}
uint32_t OperationBase::countKey(const std::string &op, const char *key, uint32_t dflt, uint32_t lo, uint32_t hi) const {
  const uint32_t v = config->getValueOr(key, dflt);
  if (v < lo || v > hi) throw std::runtime_error(op + ": " + key + " = " + S(v) + ", must be in [" + S(lo) + ", " + S(hi) + "]");
  return v;
}
std::vector<uint64_t> OperationBase::synth(uint64_t stream, bool nonZero, bool negated) const {
  std::vector<uint64_t> v;
  for (uint32_t j = 0; j < level_; ++j) {
    const uint64_t w = synthWord0(stream + j, arch->modulus(j));
    v.push_back(nonZero && w == 0 ? 1 : negated && w ? arch->modulus(j) - w : w);
  }
  return v;
}
void OperationBase::keep(const std::string &name, const std::vector<INSGROUP> &recs, bool nonZero, bool negated) {
  ConstantStage &cs = constantStages[name];
  cs.enabled = true;
  cs.nonZero = nonZero;
  cs.negated = negated;
  cs.records.resize(level_);
  for (uint32_t j = 0; j < level_; ++j) cs.records[j].push_back(recs[j][0]);
}
Limbs OperationBase::eweStage(const std::string &key, ewe_opcode op, const std::string &buffer, const Limbs &a, const Limbs *c,
                              const std::vector<uint64_t> &constants, const std::vector<AddrType> &b) {
  PerLimb s{label + "_" + key + "_Level(", ")", range(0, level_), alloc(buffer, level_)};
  s.a = a.addr;
  s.b = b;
  if (!a.from.empty()) s.after.push_back(&a.from);
  if (c) {
    s.c = c->addr;
    if (!c->from.empty()) s.after.push_back(&c->from);
  }
  s.constants = constants;
  Limbs out{s.out, eweLimbs(&insgener, op, s)};
  driver.dispatchInstructions(key, out.from);
  return out;
}
std::array<Limbs, 3> OperationBase::tensorProduct(const TensorCompute &tcm, FusedForm mark) {
  for (const INSGROUP &g : tcm.getInsMap().at("TensorCompute_INS_D1")) g[0]->mark = mark;
  std::array<Limbs, 3> d;
  for (uint32_t i = 0; i < 3; ++i) d[i] = {tcm.d(i), tcm.getInsMap().at("TensorCompute_INS_D" + S(i))};
  return d;
}
std::array<std::vector<AddrType>, 3> OperationBase::addrs(const std::array<Limbs, 3> &d) { return {d[0].addr, d[1].addr, d[2].addr}; }
void OperationBase::scaleTriple(std::array<Limbs, 3> &d, const std::string &key, const std::string &buffer, const std::string &suffix,
                                const std::string &constants, uint64_t stream) {
  for (uint32_t i = 0; i < 3; ++i) {
    d[i] = eweStage(key + "_D" + S(i), EWE_MUL_CONST, buffer + "D" + S(i) + "Scale" + suffix, d[i], nullptr, synth(stream, /*nonZero=*/true));
    keep(constants, d[i].from, /*nonZero=*/true);
  }
}
void OperationBase::addendTail(std::array<Limbs, 3> &d, const std::string &op, const std::string &buffer, const std::string &sumWord, uint32_t A,
                               uint32_t firstCt, uint64_t stream, uint64_t step, bool shifted, uint64_t constStream) {
  for (uint32_t t = 1; t <= A; ++t)
    for (uint32_t k = 0; k < 2; k++) {
      const std::string C = "_C" + S(k);
      const Limbs term = eweStage(op + "_AddScale_(" + S(t) + ")" + C, EWE_MUL_CONST, buffer + "AddScaled(" + S(t) + ")" + C, {component(firstCt + t - 1, k), {}},
                                  nullptr, synth(stream + step * t));
      keep("addscale" + S(t), term.from);
      d[k] = eweStage(op + "_Add_(" + S(t) + ")_D" + S(k), EWE_ADD, buffer + "D" + S(k) + sumWord + "(" + S(t) + ")", d[k], &term);
    }
  if (shifted) {
    d[0] = eweStage(op + "_Const_D0", EWE_ADD_CONST, buffer + "D0Const", d[0], nullptr, synth(constStream));
    keep("const", d[0].from);
  }
}
Limbs OperationBase::scaledSum(uint32_t k, uint32_t T, bool constHere, const ScaledSumNames &n) {
  const std::string C = "_C" + S(k);
  Limbs sum;
  for (uint32_t t = 1; t <= T; ++t) {
    const std::string at = n.index + S(t) + ")";
    const bool lastScale = T == 1 && !constHere, lastAdd = t == T && !constHere;
    const Limbs scaled = eweStage(n.op + "_Scale_" + at + C, EWE_MUL_CONST, lastScale ? n.result : n.op + "Scaled" + at + C, {component(t - 1, k), {}}, nullptr,
                                  synth(n.stream + n.step * t));
    keep(n.scale + S(t), scaled.from);
    if (t == 1) {
      for (const INSGROUP &g : scaled.from) g[0]->mark = FusedForm::Lincomb;
      sum = scaled;
      continue;
    }
    sum = eweStage(n.op + "_Add_" + at + C, EWE_ADD, lastAdd ? n.result : n.op + "Sum" + at + C, sum, &scaled);
  }
  if (constHere) {
    sum = eweStage(n.constKey + C, EWE_ADD_CONST, n.result, sum, nullptr, synth(n.constStream));
    keep(n.constName, sum.from);
  }
  return sum;
}
void OperationBase::finishRotation(const std::string &out, const std::vector<AddrType> &rotatedC0, const KeySwitch::Output &ks, const std::string &suffix) {
  PerLimb s{label + "_HROTATEadd" + suffix + "_Level(", ")", range(0, level_), alloc("HROTATEOutput" + suffix + "(1)", level_)};
  s.a = ks[0];
  s.c = rotatedC0;
  driver.dispatchInstructions("HROTATE_Hadd" + suffix, eweLimbs(&insgener, EWE_ADD, s));
  setOutput(out, 0, s.out);
  setOutput(out, 1, ks[1]);
}
// The sums on the extended basis (HLINTRANS, HROTSUM, HBSGS): t = 0, 1 (S_0, S_1: the key product's two components, E = level + alpha limbs) and
// t = 2 (U: the rotated c0, the `level` Q limbs), by the tags their buffers and stage keys carry
static const char *const kSumTags[4] = {"Key0", "Key1", "C0", "C1"};   // C1: W, the identity step's unrotated c1 term (the Q limbs, as C0)
std::vector<uint32_t> OperationBase::sumMods(uint32_t t) const {
  std::vector<uint32_t> mods = range(0, level_);
  if (t < 2)
    for (uint32_t p : range(maxLevel_, alpha_)) mods.push_back(p);
  return mods;
}
// sum_r terms[r] * pts[r] (t = 2: the Q limbs of pts[r]): MUL, then one MAC_ADD per further rotation, the last into LinTransOut_<tag><suffix>.  The
// term is operand a: pass (6) pairs chains that share their a operands into key products, and the plaintexts are shared by all three sums
Limbs OperationBase::weightedSum(uint32_t t, const std::vector<Limbs> &terms, const std::vector<std::vector<AddrType>> &pts, const std::string &suffix,
                                 const Limbs *head, const std::vector<AddrType> *headPt) {
  const std::string tag = kSumTags[t];
  const std::vector<uint32_t> mods = sumMods(t);
  const size_t first = head ? 0 : 1, R = terms.size() + 1;   // rotation `first` .. R - 1; 0: the unrotated head term
  Limbs sum;
  for (size_t r = first; r < R; ++r) {
    const Limbs &term = r ? terms[r - 1] : *head;
    const std::vector<AddrType> &pt = r ? pts[r - 1] : *headPt;
    const std::string at = "(" + S(r) + ")_" + tag + suffix;
    PerLimb s{label + "_LinTrans" + suffix + "_" + tag + "_Rot(" + S(r) + ")_Level(", ")", mods,
              alloc(r + 1 < R ? "LinTransOut_temp" + at : "LinTransOut_" + tag + suffix, (uint32_t)mods.size())};
    s.a = term.addr;
    s.b = t < 2 ? pt : slice(pt, 0, level_);
    if (!term.from.empty()) s.after = {&term.from};   // (the head term may be an op input: nothing to wait for)
    const Limbs before = sum;
    if (r > first) {
      s.c = before.addr;
      s.after.push_back(&before.from);
    }
    sum = {s.out, eweLimbs(&insgener, r > first ? EWE_MAC_ADD : EWE_MUL, s)};
    driver.dispatchInstructions("LinTrans_" + at, sum.from);
  }
  return sum;
}
// sum + term, the i-th: one ADD into <stem>_(<i>)_<tag>, the last into <stem>Out_<tag>
Limbs OperationBase::addTerm(uint32_t t, const Limbs &sum, const Limbs &term, const std::string &stem, uint32_t i, bool last) {
  const std::string tag = kSumTags[t], at = "(" + S(i) + ")_" + tag;
  const std::vector<uint32_t> mods = sumMods(t);
  PerLimb s{label + "_" + stem + "_" + tag + "_Ct(" + S(i) + ")_Level(", ")", mods, alloc(last ? stem + "Out_" + tag : stem + "_" + at, (uint32_t)mods.size())};
  s.a = sum.addr;
  s.c = term.addr;
  s.after = {&sum.from, &term.from};
  const Limbs out{s.out, eweLimbs(&insgener, EWE_ADD, s)};
  driver.dispatchInstructions(stem + "_" + at, out.from);
  return out;
}
// the ciphertext (U + ModDown(S_0), ModDown(S_1)) of the sums: stages <op>_Hadd<suffix> behind the ModDown's, c0 in `buffer`
OperationBase::SwitchedSum OperationBase::sumDown(KeySwitch &ks, const std::array<Limbs, 3> &sums, const std::string &op, const std::string &buffer,
                                                  const std::string &suffix, const Limbs *c1Addend) {
  const KeySwitch::Output down = ks.modDown({sums[0], sums[1]}, suffix);
  dispatch(ks.takeStages());
  PerLimb s{label + "_" + op + "add" + suffix + "_Level(", ")", range(0, level_), alloc(buffer, level_)};
  s.a = down[0];
  s.c = sums[2].addr;
  const Limbs c0{s.out, eweLimbs(&insgener, EWE_ADD, s)};
  driver.dispatchInstructions(op + "_Hadd" + suffix, c0.from);
  if (c1Addend) {   // the same stage shape as c0's
    PerLimb s1{label + "_" + op + "add1" + suffix + "_Level(", ")", range(0, level_), alloc(op + "Output" + suffix + "(1)", level_)};
    s1.a = down[1];
    s1.c = c1Addend->addr;
    const Limbs c1{s1.out, eweLimbs(&insgener, EWE_ADD, s1)};
    driver.dispatchInstructions(op + "_Hadd1" + suffix, c1.from);
    return {c0, c1.addr};
  }
  return {c0, down[1]};
}
void OperationBase::setOutput(const std::string &out, const SwitchedSum &ct, bool rescale) {
  if (rescale) return setRescaledOutput(out, {ct.c0.addr, ct.c1});
  setOutput(out, 0, ct.c0.addr);
  setOutput(out, 1, ct.c1);
}
void OperationBase::finishConstruction() {
  for (const std::string &n : addrManager->names()) arch->registerLimbs(addrManager->getAddr(n));
}
std::vector<AddrType> OperationBase::bufferAddrs(const std::string &name) const {
  auto i = namedInputs.find(name);
  if (i != namedInputs.end()) return i->second;
  auto o = namedOutputs.find(name);
  if (o != namedOutputs.end()) return o->second;
  return addrManager->getAddr(name);
}
std::vector<std::string> OperationBase::bufferNames() const {
  std::vector<std::string> v;
  for (auto &kv : namedInputs) v.push_back(kv.first);
  for (auto &kv : namedOutputs) v.push_back(kv.first);
  for (auto &n : addrManager->names()) v.push_back(n);
  return v;
}
bool OperationBase::readBuffer(const std::string &name, uint64_t *host, uint32_t copy) { return arch->readLimbs(bufferAddrs(name), host, copy); }
bool OperationBase::writeBuffer(const std::string &name, const uint64_t *host, uint32_t copy) { prepare(); return arch->writeLimbs(bufferAddrs(name), host, copy); }
void OperationBase::encodePlaintext(const std::string &name, const std::vector<std::complex<double>> &slots, double scale, uint32_t copy) {
  auto pt = plaintextMods.find(name);
  if (pt == plaintextMods.end()) {
    const bool known = namedInputs.count(name) || namedOutputs.count(name) || [&] { for (auto &n : addrManager->names()) if (n == name) return true; return false; }();
    throw std::runtime_error("encode_plaintext: " + opName + (known ? " buffer " + name + " is no plaintext input" : " has no buffer " + name));
  }
  if (slots.size() != N / 2) throw std::runtime_error("encode_plaintext: " + std::to_string(slots.size()) + " slots given, the ring has " + std::to_string(N / 2));
  static_assert(sizeof(std::complex<double>) == 2 * sizeof(double), "std::complex<double> is (re, im)");
  arch->encodeLimbs(namedInputs.at(name), pt->second, reinterpret_cast<const double *>(slots.data()), scale, copy);
}
unsigned long long OperationBase::totalInstructions() { prepare(); return driver.getTotalIns(); }
void OperationBase::bindInput(const std::string &input, OperationBase *producer, const std::string &output) {
  for (const char *part : {".c0", ".c1"}) {
    auto in = namedInputs.find(input + part);
    auto out = producer->namedOutputs.find(output + part);
    if (in == namedInputs.end()) throw std::runtime_error(opName + " has no input ciphertext " + input);
    if (out == producer->namedOutputs.end())
      throw std::runtime_error(producer->opName + (output == "out" ? " has no output ciphertext" : " has no output ciphertext " + output));
    arch->bindInput(in->second, producer->arch, out->second);
  }
}
uint32_t OperationBase::outputLevel() const {
  auto o = namedOutputs.find("out.c0");
  if (o == namedOutputs.end()) throw std::runtime_error(opName + " has no output ciphertext");
  return (uint32_t)o->second.size();
}

void OperationBase::prepare() {
  driver.IssueInsFromDramToChip(arch);
  arch->prepare();
}
double OperationBase::execute(uint32_t iters) {
  prepare();
  return arch->timedRun(iters);
}

// reference: HMULT::simulate src/Operation.cpp:1025-1112 (the five simulate() bodies are textual copies).
// The stdout contract is kept: banner, start time, [progress], completion block, stat
// block.  There is no per-cycle loop to report on; each update() launches one stage on the GPU.
// backend = sim: the reference's loop itself (src/Operation.cpp:1046-1087), on the build's own cycle model
bool OperationBase::simulateCycles(bool verbose) {
  if (arch->backend() != Arch::BACKEND_SIM) throw std::runtime_error("simulateCycles: backend is not sim");
  driver.IssueInsFromDramToChip(arch);
  arch->loadSim(buildSimProgram(opName, label, level_, alpha_, config, *addrManager, namedInputs));
  const unsigned long long TotalIns = driver.getTotalIns();
  if (arch->simModel()->totalIns() != TotalIns)
    throw std::runtime_error("sim backend: literal program has " + std::to_string(arch->simModel()->totalIns()) + " instructions, the stage graph accounts for " + std::to_string(TotalIns));
  unsigned long long exeInsCycle = 0, traced = ~0ull;
  const bool trace = getenv("HOMULATOR_SIM_TRACE") != nullptr;  // "<cycle> <retired>" whenever the count moves (oracle/ref_dump.cpp prints the same)
  time_t periodTime = time(0);
  while (!arch->simulateComplete()) {
    driver.IssueDataFromDramToChip(arch->getMemController());
    arch->update();
    const unsigned long long cycle = arch->getCycle();
    if (trace && arch->getcompletedIns() != traced) {
      traced = arch->getcompletedIns();
      std::fprintf(stderr, "%llu %llu\n", cycle, traced);
    }
    if (cycle % 2000 == 0) {
      const unsigned long long exeins = arch->getcompletedIns() - exeInsCycle;
      if (exeins == 0) {
        if (verbose) {
          std::cout << "We have executed " << exeins << " instruction(s) in this period!\n";
          arch->state();
          std::cout << "\n";
        }
        return false;
      }
      if (verbose) {
        std::cout << "\nFHE-Sim running " << cycle << " cycles!\n";
        std::cout << "We have executed " << arch->getcompletedIns() << " instructions!\n";
        const unsigned long long remainIns = TotalIns - arch->getcompletedIns();
        std::cout << "Remaining " << remainIns << " instructions!\n";
        std::cout << "We have executed " << exeins << " instruction(s) in this period!\n";
        const time_t nowTime = time(0);
        const double speed = static_cast<double>(exeins) / (nowTime - periodTime);
        std::cout << "Estimated time remaining " << static_cast<double>(remainIns) / speed / 60 << " minutes\n";
        periodTime = nowTime;
      }
      exeInsCycle = arch->getcompletedIns();
    }
  }
  return true;
}

bool OperationBase::simulate() {
  const bool sim = arch->backend() == Arch::BACKEND_SIM;
  if (!sim) driver.IssueInsFromDramToChip(arch);
  std::cout << "\n\nWelcome! Start simulating " << opName << "!\n\n";
  time_t t0 = time(0);
  std::cout << "Start time: " << ctime(&t0) << std::endl;
  if (sim) {
    simulateCycles(true);
  } else {
    arch->prepare();
    arch->run();   // untimed warm-up of the whole plan (first-use table uploads, code-object loads); the plan is idempotent
    arch->sync();
    while (!arch->simulateComplete()) {
      driver.IssueDataFromDramToChip(arch->getMemController());
      arch->update();
    }
    arch->sync();
    std::cout << "\nFHE-Sim running " << arch->getCycle() << " cycles!\n";  // unit: device nanoseconds (see Arch.h)
    std::cout << "We have executed " << arch->getcompletedIns() << " instructions!\n";
    std::cout << "Remaining " << driver.getTotalIns() - arch->getcompletedIns() << " instructions!\n";
  }
  time_t t1 = time(0);
  std::cout << "\n\nCompleted Simulate!\n";
  std::cout << "FHE-Sim Total simulated\t" << arch->getCycle() << " cycles!\n\n";
  std::cout << "End time: " << ctime(&t1) << std::endl;
  std::cout << "The simulator total cost\t" << static_cast<double>(t1 - t0) / 60 << " Minutes!\n";
  arch->shownStat();
  return true;
}

// =====================================================================================================
// op classes
// =====================================================================================================
// reference: HMULT::HMULT :913-1023.  Wiring: KS(d2); out0 = d0 + ks0; out1 = d1 + ks1 (Appendix C item 1)
HMULT::HMULT(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HMULT", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  makeInputs(2);
  TensorCompute tcm(labelName, currentLevel, &cts[0], &cts[1], &Datapool, &DataInsMap, &insgener, addrManager.get());
  dispatch(tcm.getInsMap());

  relinearizeAndRescale({tcm.d(0), tcm.d(1), tcm.d(2)});
  finishConstruction();
}

// reference: HROTATE::HROTATE :1271-1358.  Wiring: c'_k = sigma_g(c_k); KS(c'_1); out0 = c'_0 + ks0; out1 = ks1
// (Appendix C item 2).  The Galois element is the config key `galois` (default 5 = rotation by one slot).
HROTATE::HROTATE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HROTATE", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  makeInputs(1);
  const uint32_t galois = cfg->getValueOr("galois", 5);
  const std::vector<AddrType> rc0 = rotateComponent(0, galois, "").addr, rc1 = rotateComponent(1, galois, "").addr;
  KeySwitch ksw(labelName, maxLevel, currentLevel, alpha, rc1, &Datapool, &DataInsMap, &insgener, addrManager.get());
  dispatch(ksw.getInsMap());
  finishRotation("out", rc0, ksw.output(), "");
  finishConstruction();
}

// hreim (build extension).  HROTATE's body with galois = 2N - 1, unchanged, into the named output conj (buffers ReImConj(k):
// HROTATE's own output buffers under that name), then per component k, existing opcodes only: ReIm_Add_C<k> = ct1.c<k> + conj.c<k> (ADD) into
// ReImOutput(k), ReIm_Sub_C<k> = ct1.c<k> - conj.c<k> (SUB) into ReImDiff(k), ReIm_Mul_C<k> = that times the buffer `unit` (MUL) into ReImOutputIm(k).
// Unfused, the three stages run as element-wise launches; fused, pass (5r) of Arch::fusePasses (Planner.cpp) turns the three records of a limb and
// component into one record of ONE launch, which does not read `unit`.  Every buffer of HROTATE is allocated first, in HROTATE's order: the
// launches in front of the tail are HROTATE's, field for field.
HREIM::HREIM(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HREIM", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hreim", "the reference has no monomial product");
  makeInputs(1);
  const uint32_t galois = 2 * N - 1;   // the conjugation; the config key galois is not read
  const std::vector<AddrType> rc0 = rotateComponent(0, galois, "").addr, rc1 = rotateComponent(1, galois, "").addr;
  KeySwitch ksw(labelName, maxLevel, currentLevel, alpha, rc1, &Datapool, &DataInsMap, &insgener, addrManager.get());
  dispatch(ksw.getInsMap());
  finishRotation("conj", rc0, ksw.output(), "");
  const std::vector<AddrType> unit = alloc("unit", currentLevel);
  arch->addUnitFill(unit, range(0, currentLevel));
  for (uint32_t k = 0; k < 2; k++) {
    const std::string C = "_C" + S(k);
    const Limbs x{component(0, k), {}}, y{namedOutputs.at("conj.c" + S(k)), {}};
    const Limbs sum = eweStage("ReIm_Add" + C, EWE_ADD, "ReImOutput(" + S(k) + ")", x, &y);
    for (const INSGROUP &g : sum.from) g[0]->mark = FusedForm::ReIm;
    const Limbs diff = eweStage("ReIm_Sub" + C, EWE_SUB, "ReImDiff(" + S(k) + ")", x, &y);
    const Limbs im = eweStage("ReIm_Mul" + C, EWE_MUL, "ReImOutputIm(" + S(k) + ")", diff, nullptr, {}, unit);
    setOutput("out", k, sum.addr);
    setOutput("out_im", k, im.addr);
  }
  finishConstruction();
}

// hrotate_hoisted (build extension: the reference has no such op).  R rotations of one ciphertext by g_r = g^r mod 2N, r = 1..R, sharing ONE
// ModUp of the UNROTATED c1 (KeySwitch::modUp): D_j = ModUp(c1).  Per rotation (stage keys and buffers suffixed _Rot<r>): AUTO of every extended
// digit (rotateDigits), the key product with the rotation's own key, the ModDown, then out<r> = (sigma_r(c0) + ks0_r, ks1_r).
// Not bit-identical to R hrotates: ModUp(sigma(c1)) and sigma(ModUp(c1)) differ by multiples of Q in the converted limbs; both key switches are
// valid.  Unfused, the stages run one launch each; fused, pass (6h) of Arch::fusePasses (Planner.cpp) turns the R key products into one hoisted launch.
HROTATE_HOISTED::HROTATE_HOISTED(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HROTATE_HOISTED", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  const std::vector<uint32_t> gs = hoistedRotations("hrotate_hoisted");
  const uint32_t R = (uint32_t)gs.size();
  makeInputs(1);

  KeySwitch ks(labelName, maxLevel, currentLevel, alpha, &Datapool, &DataInsMap, &insgener, addrManager.get());
  const KeySwitch::Digits digits = ks.modUp(cts[0].getC1Addr(), /*inputMayBeOpInput=*/true);
  dispatch(ks.takeStages());
  for (uint32_t r = 1; r <= R; ++r) {
    const std::string rs = "_Rot" + S(r);
    // rotation r's key: the synthetic stream seed + 10000 + 100000 r (+ (2 j + k) 1000 per digit and component, as IP_Key<k>_<j>)
    const KeySwitch::Output out = ks.modDown(ks.keyProduct(ks.rotateDigits(digits, gs[r - 1], rs), seed + 10000 + 100000ull * r, rs), rs);
    dispatch(ks.takeStages());
    finishRotation("out" + S(r), rotateComponent(0, gs[r - 1], rs).addr, out, rs);
  }
  finishConstruction();
}

// hlintrans (build extension).  out = sum_r pt_r (.) rot_r(ct1) over hrotate_hoisted's R rotations, with its shared ModUp D_j = ModUp(c1) and ONE
// ModDown: the plaintexts pt<r> live on the extended basis, multiplying by them and the ModDown are both linear, so the weighted sum is formed
// on the E = l + alpha limbs first:
//   acc_{r,k} = sum_j sigma_r(D_j) evk_r[j][k]       rotateDigits + keyProduct per rotation, as hrotate_hoisted
//   S_k = sum_r acc_{r,k} pt_r   (E limbs),   U = sum_r sigma_r(c0) pt_r[Q limbs]   (l limbs)        MUL, then MAC_ADD per further rotation
//   out.c0 = U + ModDown(S_0),   out.c1 = ModDown(S_1)
// A valid key switch, not bit-identical to hrotate_hoisted + R pmult + R - 1 hadd (that rounds in R ModDowns, this in one).  Unfused, the stages
// run one launch each; fused, pass (6l) of Arch::fusePasses (Planner.cpp) turns everything between the ModUp and the ModDown into one launch.
HLINTRANS::HLINTRANS(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HLINTRANS", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  const std::vector<uint32_t> gs = hoistedRotations("hlintrans");
  const uint32_t R = (uint32_t)gs.size();
  // identity = 1: one more plaintext pt0 (stream seed + 4300) weights the UNROTATED ciphertext, which meets no key:
  //   U = pt0[Q] c0 + sum_r pt_r[Q] sigma_r(c0),   W = pt0[Q] c1,   out.c1 = W + ModDown(S_1)
  // 16 terms per accumulator at most, so rotations <= 15
  const bool identity = identityStep("hlintrans"), rescale = rescaleKey("hlintrans");
  if (identity && R > 15) throw std::runtime_error("hlintrans: rotations = " + S(R) + " with identity = 1, must be in [1, 15]");
  makeInputs(1, /*plaintext=*/false, /*extPlaintexts=*/R, identity ? NamedStreams{{"pt0", 4300}} : NamedStreams{});

  KeySwitch ks(labelName, maxLevel, currentLevel, alpha, &Datapool, &DataInsMap, &insgener, addrManager.get());
  const KeySwitch::Digits digits = ks.modUp(cts[0].getC1Addr(), /*inputMayBeOpInput=*/true);
  dispatch(ks.takeStages());
  std::array<std::vector<Limbs>, 3> terms;          // per rotation: acc_{r,0}, acc_{r,1}, sigma_r(c0)
  std::vector<std::vector<AddrType>> pts;           // ... and the plaintext they meet
  for (uint32_t r = 1; r <= R; ++r) {
    const std::string rs = "_Rot" + S(r);
    const KeySwitch::Accumulators acc = ks.keyProduct(ks.rotateDigits(digits, gs[r - 1], rs), seed + 10000 + 100000ull * r, rs);
    dispatch(ks.takeStages());
    terms[0].push_back(acc[0]); terms[1].push_back(acc[1]); terms[2].push_back(rotateComponent(0, gs[r - 1], rs));
    pts.push_back(namedInputs.at("pt" + S(r)));
  }
  std::array<Limbs, 3> sums;
  if (!identity) {
    for (uint32_t t = 0; t < 3; ++t) sums[t] = weightedSum(t, terms[t], pts, "");
    setOutput("out", sumDown(ks, sums, "HLINTRANS", "HLINTRANSOutput(0)", ""), rescale);
  } else {
    const Limbs c0{cts[0].getC0Addr(), {}}, c1{cts[0].getC1Addr(), {}};
    const std::vector<AddrType> &pt0 = namedInputs.at("pt0");
    for (uint32_t t = 0; t < 2; ++t) sums[t] = weightedSum(t, terms[t], pts, "");
    sums[2] = weightedSum(2, terms[2], pts, "", &c0, &pt0);
    const Limbs W = weightedSum(3, {}, {}, "", &c1, &pt0);
    setOutput("out", sumDown(ks, sums, "HLINTRANS", "HLINTRANSOutput(0)", "", &W), rescale);
  }
  finishConstruction();
}

// hdot (build extension).  out = Rescale(d0 + ks0(d2)), Rescale(d1 + ks1(d2)) with d_i = sum_t d_i,t over the T pairs (ct<2t-1>, ct<2t>): the
// tensor product, the key switch and the rescale are linear in (d0, d1, d2), so ONE relinearisation and ONE rescale serve the whole sum.  Pair 1
// runs TensorCompute's three stages; pair t >= 2 adds its products onto the running sums, d0 += c00 c10 and d2 += c01 c11 (MAC_ADD), d1 += c00 c11 +
// c01 c10 (MAC2 into a per-pair temporary, then ADD); the last pair writes DotD<i>Out.  Then HMULT's tail, stage for stage.  Every sum is the
// canonical residue of the exact integer sum: bit-identical to tensor + EWE_ADD of the d's + hmult's tail, and to hmult at T = 1.  Unfused, the
// stages run one launch each; fused, pass (5d) of Arch::fusePasses (Planner.cpp) turns everything in front of the key switch into one launch.
HDOT::HDOT(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HDOT", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hdot", "the reference has no sum of products");
  const uint32_t T = countKey("hdot", "terms", 4, 1, 16);
  makeInputs(2 * T);
  auto name = [&](uint32_t i, uint32_t pair) { return "DotD" + S(i) + "Out" + (pair < T ? "_temp(" + S(pair) + ")" : ""); };   // pair: 1-based

  TensorCompute tcm(labelName, currentLevel, &cts[0], &cts[1], &Datapool, &DataInsMap, &insgener, addrManager.get(), "Dot", T > 1 ? "_temp(1)" : "");
  std::array<Limbs, 3> d = tensorProduct(tcm, FusedForm::TensorDot);
  dispatch(tcm.getInsMap());
  for (uint32_t p = 2; p <= T; ++p) {
    const std::vector<AddrType> c00 = component(2 * p - 2, 0), c01 = component(2 * p - 2, 1), c10 = component(2 * p - 1, 0), c11 = component(2 * p - 1, 1);
    const std::string at = "_Pair(" + S(p) + ")_Level(";
    auto emit = [&](const std::string &key, ewe_opcode op, const PerLimb &s) {
      Limbs out{s.out, eweLimbs(&insgener, op, s)};
      driver.dispatchInstructions(key + "_(" + S(p) + ")", out.from);
      return out;
    };
    const std::array<Limbs, 3> before = d;
    PerLimb s0{labelName + "_Dot_D0" + at, ")", range(0, currentLevel), alloc(name(0, p), currentLevel)};   // d0 += c00 c10
    s0.a = c00; s0.b = c10; s0.c = before[0].addr; s0.after = {&before[0].from};
    d[0] = emit("Dot_D0", EWE_MAC_ADD, s0);
    PerLimb m1{labelName + "_Dot_D1Mac" + at, ")", s0.mods, alloc("DotD1Mac(" + S(p) + ")", currentLevel)};   // c00 c11 + c01 c10
    m1.a = c00; m1.b = c11; m1.c = c01; m1.d = c10;
    const Limbs mac = emit("Dot_D1Mac", EWE_MAC2, m1);
    PerLimb s1{labelName + "_Dot_D1" + at, ")", s0.mods, alloc(name(1, p), currentLevel)};                    // d1 += that
    s1.a = before[1].addr; s1.c = mac.addr; s1.after = {&before[1].from, &mac.from};
    d[1] = emit("Dot_D1", EWE_ADD, s1);
    PerLimb s2{labelName + "_Dot_D2" + at, ")", s0.mods, alloc(name(2, p), currentLevel)};                    // d2 += c01 c11
    s2.a = c01; s2.b = c11; s2.c = before[2].addr; s2.after = {&before[2].from};
    d[2] = emit("Dot_D2", EWE_MAC_ADD, s2);
  }

  relinearizeAndRescale(addrs(d));   // HMULT's tail, on the sums
  finishConstruction();
}

// hsquare (build extension).  out = Rescale(d0 + ks0(d2)), Rescale(d1 + ks1(d2)) with d0 = s a a + k, d1 = 2 s a c, d2 = s c c
// (a = ct1.c0, c = ct1.c1).  TensorCompute on (ct1, ct1): its MAC2 a c + c a is 2 a c and its MULs are the squares; sq_scale = 1 adds three MUL_CONST
// stages (s on d0, d1, d2: linear, so it acts in front of the key switch), sq_const = 1 one ADD_CONST stage on d0 (the constant polynomial k in
// evaluation form, where an FHE library adds it, at scale Delta^2).  Then HMULT's tail, stage for stage.  Unfused, the stages run one launch each;
// fused, pass (5q) of Arch::fusePasses (Planner.cpp) turns everything in front of the key switch into one launch that reads ct1 once.
HSQUARE::HSQUARE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HSQUARE", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hsquare", "the reference has no square");
  const bool scaled = flag("hsquare", "sq_scale"), shifted = flag("hsquare", "sq_const");
  makeInputs(1);

  TensorCompute tcm(labelName, currentLevel, &cts[0], &cts[0], &Datapool, &DataInsMap, &insgener, addrManager.get(), "Sq");
  std::array<Limbs, 3> d = tensorProduct(tcm, FusedForm::Square);
  dispatch(tcm.getInsMap());
  constantStages["scale"].key = "sq_scale";
  constantStages["const"].key = "sq_const";
  if (scaled) scaleTriple(d, "Square_Scale", "Sq", "", "scale", seed + 6000);
  if (shifted) {
    d[0] = eweStage("Square_Const_D0", EWE_ADD_CONST, "SqD0Const", d[0], nullptr, synth(seed + 6100));
    keep("const", d[0].from);
  }
  relinearizeAndRescale(addrs(d));
  finishConstruction();
}

// hlincomb (build extension).  Per component k, with x_t = ct<t>.c<k>: LinComb_Scale_(t)_C<k> = s_t x_t (MUL_CONST) for every t,
// LinComb_Add_(t)_C<k> = the running sum plus term t (ADD) for t >= 2, and with lc_const = 1 LinComb_Const_C0 = the sum of c0 plus k (ADD_CONST: the
// constant polynomial in evaluation form, on c0 only as PADD's plaintext).  The last buffer of a component is LinCombOutput(k).  Unfused, the stages
// run as element-wise launches; fused, pass (5l) of Arch::fusePasses (Planner.cpp) turns each limb's chain into one record of ONE launch.
HLINCOMB::HLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HLINCOMB", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hlincomb", "the reference has no scalar product");
  const uint32_t T = countKey("hlincomb", "terms", 4, 1, 16);
  const bool shifted = flag("hlincomb", "lc_const"), rescale = rescaleKey("hlincomb");
  makeInputs(T);
  constantStages["const"].key = "lc_const";
  std::array<std::vector<AddrType>, 2> out;   // both components share the scalars
  for (uint32_t k = 0; k < 2; k++)
    out[k] = scaledSum(k, T, shifted && k == 0, {"LinComb", "(", "LinCombOutput(" + S(k) + ")", "LinComb_Const", "scale", "const", seed + 6200, 100, seed + 6290}).addr;
  if (rescale) setRescaledOutput("out", out);
  else for (uint32_t k = 0; k < 2; k++) setOutput("out", k, out[k]);
  finishConstruction();
}

// hmlincomb (build extension).  For every output m, HLINCOMB's stages from existing opcodes only.  Per component k, with
// x_t = ct<t>.c<k>: MLinComb_Scale_(m,t)_C<k> = s_{m,t} x_t (MUL_CONST) for every t, MLinComb_Add_(m,t)_C<k> = the running sum plus term t (ADD)
// for t >= 2, and with ml_const = 1 MLinComb_Const_(m)_C0 = the sum of c0 plus k_m (ADD_CONST).  The last buffer of a sum is MLinCombOutput(m,k).
// Every sum is emitted before any rescale, so that nothing reads an output in front of the last sum.  Unfused, the stages run as element-wise
// launches; fused, pass (5l) turns each (m, limb, component) chain into one record and pass (5L) merges the M records over one list of inputs
// into one record of ONE hm_lincomb_multi launch (Planner.cpp); fuse_mlincomb = 0 leaves them to (5l)'s launch.
HMLINCOMB::HMLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HMLINCOMB", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hmlincomb", "the reference has no scalar product");
  const uint32_t T = countKey("hmlincomb", "terms", 4, 1, 16), M = countKey("hmlincomb", "outputs", 4, 1, 16);
  const bool shifted = flag("hmlincomb", "ml_const");
  flag("hmlincomb", "fuse_mlincomb", 1);
  const bool rescale = rescaleKey("hmlincomb");
  if (rescale && currentLevel < 2) throw std::runtime_error("hmlincomb: Rescale needs at least two limbs");
  makeInputs(T);
  std::vector<std::array<std::vector<AddrType>, 2>> outs(M);
  for (uint32_t m = 1; m <= M; ++m) {
    constantStages["const" + S(m)].key = "ml_const";
    const uint64_t streams = seed + 8000 + 1000ull * m;
    for (uint32_t k = 0; k < 2; k++)
      outs[m - 1][k] = scaledSum(k, T, shifted && k == 0, {"MLinComb", "(" + S(m) + ",", "MLinCombOutput(" + S(m) + "," + S(k) + ")", "MLinComb_Const_(" + S(m) + ")",
                                                           "scale" + S(m) + "_", "const" + S(m), streams + 100, 50, streams + 950}).addr;
  }
  for (uint32_t m = 1; m <= M; ++m)
    for (uint32_t k = 0; k < 2; k++) {
      std::vector<AddrType> out = outs[m - 1][k];
      if (rescale) {   // setRescaledOutput's builder, with a label of its own per output
        Rescale res(label + "_Out" + S(m) + "_" + S(k), level_, out, &Datapool, &DataInsMap, &insgener, addrManager.get());
        dispatch(res.getInsMap());
        out = res.output();
      }
      setOutput("out" + S(m), k, out);
      if (m == 1) setOutput("out", k, out);   // "out" names out1: the op is a legal link of a chain
    }
  finishConstruction();
}

// hclincomb (build extension).  Per component k and term t, with x_t = ct<t>.c<k>, existing opcodes only, `unit` being HREIM's
// named buffer U = -X^(N/2) in evaluation form (Arch::addUnitFill), so that +X^(N/2) b is U (q - b mod q):
//   CLinComb_Re_(t)_C<k> = a_t x_t (MUL_CONST),  CLinComb_Rot_(t)_C<k> = x_t (.) unit (MUL),  CLinComb_Im_(t)_C<k> = that times (q - b_t) mod q (MUL_CONST),
//   CLinComb_Term_(t)_C<k> = Re + Im (ADD),  CLinComb_Add_(t)_C<k> = the running sum plus the term (ADD) for t >= 2,
// and with cl_const = 1 CLinComb_Const_C0 = the sum of c0 plus k (ADD_CONST, on c0 only as PADD's plaintext).  The last buffer of a component is
// CLinCombOutput(k).  Unfused, the stages run as element-wise launches; fused, pass (5c) of Arch::fusePasses (Planner.cpp) turns each limb's chain
// into one record of ONE launch, which does not read `unit`.
HCLINCOMB::HCLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HCLINCOMB", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hclincomb", "the reference has no monomial product");
  const uint32_t T = countKey("hclincomb", "terms", 4, 1, 16);
  const bool shifted = flag("hclincomb", "cl_const"), rescale = rescaleKey("hclincomb");
  makeInputs(T);
  constantStages["const"].key = "cl_const";
  const std::vector<AddrType> unit = alloc("unit", currentLevel);
  arch->addUnitFill(unit, range(0, currentLevel));
  std::array<std::vector<AddrType>, 2> out;   // both components share the scalars
  for (uint32_t k = 0; k < 2; k++) {
    const std::string C = "_C" + S(k), result = "CLinCombOutput(" + S(k) + ")";
    const bool constHere = shifted && k == 0;
    Limbs sum;
    for (uint32_t t = 1; t <= T; ++t) {
      const std::string at = "_(" + S(t) + ")" + C;
      const Limbs x{component(t - 1, k), {}};
      const Limbs real = eweStage("CLinComb_Re" + at, EWE_MUL_CONST, "CLinCombRe" + at, x, nullptr, synth(seed + 6450 + 100ull * t));
      keep("scale" + S(t), real.from);
      if (t == 1)
        for (const INSGROUP &g : real.from) g[0]->mark = FusedForm::CLincomb;
      const Limbs rot = eweStage("CLinComb_Rot" + at, EWE_MUL, "CLinCombRot" + at, x, nullptr, {}, unit);
      // the monomial part carries q - value: the stored factor is -X^(N/2)
      const Limbs imag = eweStage("CLinComb_Im" + at, EWE_MUL_CONST, "CLinCombIm" + at, rot, nullptr, synth(seed + 8150 + 100ull * t, false, /*negated=*/true));
      keep("scale_im" + S(t), imag.from, false, /*negated=*/true);
      const Limbs term = eweStage("CLinComb_Term" + at, EWE_ADD, T == 1 && !constHere ? result : "CLinCombTerm" + at, real, &imag);
      sum = t == 1 ? term : eweStage("CLinComb_Add" + at, EWE_ADD, t == T && !constHere ? result : "CLinCombSum" + at, sum, &term);
    }
    if (constHere) {
      sum = eweStage("CLinComb_Const" + C, EWE_ADD_CONST, result, sum, nullptr, synth(seed + 9850));
      keep("const", sum.from);
    }
    out[k] = sum.addr;
  }
  if (rescale) setRescaledOutput("out", out);
  else for (uint32_t k = 0; k < 2; k++) setOutput("out", k, out[k]);
  finishConstruction();
}

// hplincomb (build extension).  Per component k, with x_t = ct<t>.c<k> and p_t = pt<t>, existing opcodes only:
//   PLinComb_Mul_(1)_C<k> = p_1 (.) x_1 (MUL),  PLinComb_Mac_(t)_C<k> = p_t (.) x_t + the running sum (MAC_ADD) for t >= 2,
// and with pl_addend = 1 PLinComb_Addend_C0 = the sum of c0 plus pt0 (ADD, on c0 only as PADD's plaintext).  The last buffer of a component is
// PLinCombOutput(k).  The ciphertext is operand a and the plaintext operand b, as PMULT's: the two chains then share no a operand, so pass (6)
// never takes them for the two keys of a key product.  Unfused, the stages run as element-wise launches; fused, pass (5p) of Arch::fusePasses
// (Planner.cpp) turns the two chains of a limb into one record of ONE launch.
HPLINCOMB::HPLINCOMB(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HPLINCOMB", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hplincomb", "the reference sums no plaintext products");
  const uint32_t T = countKey("hplincomb", "terms", 4, 1, 16);
  const bool addend = flag("hplincomb", "pl_addend"), rescale = rescaleKey("hplincomb");
  NamedStreams pts;
  for (uint32_t t = 1; t <= T; ++t) pts.push_back({"pt" + S(t), 4000 + 100000ull * t});
  if (addend) pts.push_back({"pt0", 4000 + 100000ull * 17});
  makeInputs(T, /*plaintext=*/false, /*extPlaintexts=*/0, NamedStreams{}, pts);
  std::array<std::vector<AddrType>, 2> out;
  for (uint32_t k = 0; k < 2; k++) {
    const std::string C = "_C" + S(k), result = "PLinCombOutput(" + S(k) + ")";
    const bool addendHere = addend && k == 0;
    Limbs sum;
    for (uint32_t t = 1; t <= T; ++t) {
      const std::string stage = std::string(t == 1 ? "PLinComb_Mul_(" : "PLinComb_Mac_(") + S(t) + ")" + C;
      sum = eweStage(stage, t == 1 ? EWE_MUL : EWE_MAC_ADD, t == T && !addendHere ? result : "PLinCombSum(" + S(t) + ")" + C, {component(t - 1, k), {}},
                     t == 1 ? nullptr : &sum, {}, namedInputs.at("pt" + S(t)));
      if (t == 1)
        for (const INSGROUP &g : sum.from) g[0]->mark = FusedForm::PLincomb;
    }
    if (addendHere) {
      const Limbs pt0{namedInputs.at("pt0"), {}};
      sum = eweStage("PLinComb_Addend" + C, EWE_ADD, result, sum, &pt0);
      for (const INSGROUP &g : sum.from) g[0]->mark = FusedForm::PLincomb;   // the addend belongs to the marked sum
    }
    out[k] = sum.addr;
  }
  if (rescale) setRescaledOutput("out", out);
  else for (uint32_t k = 0; k < 2; k++) setOutput("out", k, out[k]);
  finishConstruction();
}

// hmuladd (build extension).  out = Rescale(d0 + ks0(d2)), Rescale(d1 + ks1(d2)) with
//   d0 = s a b + sum_t u_t x_t + k,  d1 = s (a d + c b) + sum_t u_t y_t,  d2 = s c d
// (a, c = ct1.c0, ct1.c1; b, d = ct2.c0, ct2.c1; x_t, y_t = ct<2+t>.c0, .c1): one node of a polynomial evaluation, T_{a+b} = 2 T_a T_b - T_{|a-b|} or
// p = q T_g + r.  TensorCompute on (ct1, ct2); ma_scale = 1 adds three MUL_CONST stages MulAdd_Scale_D<i> (s on d0, d1, d2); per addend t and
// component k MulAdd_AddScale_(t)_C<k> = u_t ct<2+t>.c<k> (MUL_CONST) and MulAdd_Add_(t)_D<k> = d<k> plus that (ADD); ma_const = 1 one ADD_CONST
// stage MulAdd_Const_D0.  Everything is linear and acts in front of the key switch, at scale Delta^2 on the level of the inputs.  Then HMULT's
// tail, stage for stage.  Unfused, the stages run one launch each; fused, pass (5m) of Arch::fusePasses (Planner.cpp) turns everything in front
// of the key switch into one launch.
HMULADD::HMULADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HMULADD", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hmuladd", "the reference has no scalar product");
  if (currentLevel < 2) throw std::runtime_error("hmuladd: Rescale needs at least two limbs");
  const uint32_t A = countKey("hmuladd", "addends", 1, 0, HM_TENSOR_MULADD_MAX_ADDENDS);
  const bool scaled = flag("hmuladd", "ma_scale"), shifted = flag("hmuladd", "ma_const");
  makeInputs(2 + A);

  TensorCompute tcm(labelName, currentLevel, &cts[0], &cts[1], &Datapool, &DataInsMap, &insgener, addrManager.get(), "Ma");
  std::array<Limbs, 3> d = tensorProduct(tcm, FusedForm::MulAdd);
  dispatch(tcm.getInsMap());
  constantStages["scale"].key = "ma_scale";
  constantStages["const"].key = "ma_const";
  if (scaled) scaleTriple(d, "MulAdd_Scale", "Ma", "", "scale", seed + 6400);
  addendTail(d, "MulAdd", "Ma", "Sum", A, /*firstCt=*/2, seed + 6400, 10, shifted, seed + 6490);
  relinearizeAndRescale(addrs(d));
  finishConstruction();
}

// hdotadd (build extension).  out = Rescale(d0 + ks0(d2)), Rescale(d1 + ks1(d2)) with
//   d0 = sum_t s_t a_t b_t + sum_r u_r x_r + k,  d1 = sum_t s_t (a_t d_t + c_t b_t) + sum_r u_r y_r,  d2 = sum_t s_t c_t d_t
// (a_t, c_t = ct<2t-1>.c0, .c1; b_t, d_t = ct<2t>.c0, .c1; x_r, y_r = ct<2T+r>.c0, .c1): one node of a polynomial evaluation with several products,
// p = sum_i q_i G_i + r, or one component of a complex product behind hreim.  Existing opcodes only, in one uniform form: per pair t TensorCompute
// into buffers of its own (DaD<i>Out_(t)); da_scale = 1 adds three MUL_CONST stages DotAdd_Scale_(t)_D<i> (s_t on the pair's d0, d1, d2); for
// t >= 2 three ADD stages DotAdd_Sum_(t)_D<i> onto the running sums; then the addends exactly as HMULADD emits them, DotAdd_AddScale_(r)_C<k> =
// u_r ct<2T+r>.c<k> (MUL_CONST) and DotAdd_Add_(r)_D<k> (ADD); da_const = 1 one ADD_CONST stage DotAdd_Const_D0.  Everything is linear and acts
// in front of the key switch, at scale Delta^2 on the level of the inputs.  Then HMULT's tail, stage for stage.  Unfused, the stages run one
// launch each; fused, pass (5a) of Arch::fusePasses (Planner.cpp) turns everything in front of the key switch into one launch.
HDOTADD::HDOTADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HDOTADD", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  refuseSimAndSharded("hdotadd", "the reference has no sum of scaled products");
  if (currentLevel < 2) throw std::runtime_error("hdotadd: Rescale needs at least two limbs");
  const uint32_t T = countKey("hdotadd", "terms", 4, 1, HM_TENSOR_DOTADD_MAX_TERMS), A = countKey("hdotadd", "addends", 1, 0, HM_TENSOR_DOTADD_MAX_ADDENDS);
  const bool scaled = flag("hdotadd", "da_scale"), shifted = flag("hdotadd", "da_const");
  flag("hdotadd", "fuse_dotadd", 1);
  makeInputs(2 * T + A);

  for (uint32_t t = 1; t <= T; ++t) constantStages["scale" + S(t)].key = "da_scale";
  constantStages["const"].key = "da_const";
  std::array<Limbs, 3> d;   // the running sums
  for (uint32_t t = 1; t <= T; ++t) {
    const std::string P = "(" + S(t) + ")";
    TensorCompute tcm(t == 1 ? labelName : labelName + "_Pair" + P, currentLevel, &cts[2 * t - 2], &cts[2 * t - 1], &Datapool, &DataInsMap, &insgener,
                      addrManager.get(), "Da", "_" + P);
    std::array<Limbs, 3> p = tensorProduct(tcm, t == 1 ? FusedForm::DotAdd : FusedForm::None);
    for (const auto &st : tcm.getInsMap()) driver.dispatchInstructions(t == 1 ? st.first : st.first + "_" + P, st.second);
    if (scaled) scaleTriple(p, "DotAdd_Scale_" + P, "Da", P, "scale" + S(t), seed + 6050 + 50ull * t);
    if (t == 1) { d = p; continue; }
    for (uint32_t i = 0; i < 3; ++i) d[i] = eweStage("DotAdd_Sum_" + P + "_D" + S(i), EWE_ADD, "DaD" + S(i) + "Sum" + P, d[i], &p[i]);
  }
  addendTail(d, "DotAdd", "Da", "Add", A, /*firstCt=*/2 * T, seed + 7050, 50, shifted, seed + 7900);   // the addends and the constant exactly as HMULADD's
  relinearizeAndRescale(addrs(d));
  finishConstruction();
}

// hrotsum (build extension).  out = sum_i rot_{g_i}(ct<i>), g_i = g^i mod 2N, over G DIFFERENT ciphertexts with ONE ModDown: the ModDown is linear,
// so the G key products are summed on the E = l + alpha limbs and brought down once (the ModUps cannot be shared: the ciphertexts differ).
//   D_{i,j} = ModUp(ct<i>.c1)                          per ciphertext, on the unrotated c1 (buffers and stages of ciphertext i >= 2 suffixed _Ct<i>)
//   acc_{i,k} = sum_j sigma_i(D_{i,j}) evk_i[j][k]     rotateDigits + keyProduct with hrotate_hoisted's key of rotation i (suffix _Rot<i>)
//   S_k = sum_i acc_{i,k}   (E limbs),   U = sum_i sigma_i(ct<i>.c0)   (l limbs)        one ADD per further ciphertext onto the running sums
//   out.c0 = U + ModDown(S_0),   out.c1 = ModDown(S_1)
// Every sum is the canonical residue of the exact integer sum.  A valid key switch, not bit-identical to G hrotate + G - 1 hadd (that rounds in
// G ModDowns, this in one); at G = 1 it is hrotate_hoisted with rotations = 1.  Unfused, the stages run one launch each; fused, pass (6s) of
// Arch::fusePasses (Planner.cpp) turns everything between the ModUps and the ModDown into one launch.
HROTSUM::HROTSUM(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HROTSUM", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  const std::vector<uint32_t> gs = hoistedRotations("hrotsum");
  const uint32_t G = (uint32_t)gs.size();
  const bool rescale = rescaleKey("hrotsum");
  makeInputs(G);

  KeySwitch ks(labelName, maxLevel, currentLevel, alpha, &Datapool, &DataInsMap, &insgener, addrManager.get());
  std::array<Limbs, 3> sums;   // S_0, S_1, U so far
  for (uint32_t i = 1; i <= G; ++i) {
    const std::string rs = "_Rot" + S(i);
    const KeySwitch::Digits digits = ks.modUp(cts[i - 1].getC1Addr(), /*inputMayBeOpInput=*/true, i == 1 ? "" : "_Ct" + S(i));
    const KeySwitch::Accumulators acc = ks.keyProduct(ks.rotateDigits(digits, gs[i - 1], rs), seed + 10000 + 100000ull * i, rs);
    dispatch(ks.takeStages());
    const std::array<Limbs, 3> term = {acc[0], acc[1], rotateComponent(0, gs[i - 1], rs, i - 1)};
    for (uint32_t t = 0; t < 3; ++t) sums[t] = i == 1 ? term[t] : addTerm(t, sums[t], term[t], "RotSum", i, i == G);
  }
  setOutput("out", sumDown(ks, sums, "HROTSUM", "HROTSUMOutput(0)", ""), rescale);
  finishConstruction();
}

// hbsgs (build extension).  The baby-step/giant-step linear transform out = sum_i rot_{h_i}( sum_r pt_{i,r} (.) rot_{g_r}(ct1) ), g_r = g^r, h_i = h^i mod 2N
// (the double-hoisted baby step of Bossuat et al. in front of hrotsum's giant step):
//   D_j = ModUp(c1)                                     ONCE, on the unrotated c1
//   acc_{r,k} = sum_j sigma_{g_r}(D_j) evk_r[j][k]      once per baby rotation (suffix _Rot<r>), hlintrans's keys
//   S_{i,k} = sum_r pt_{i,r} acc_{r,k}   (E limbs),   U_i = sum_r pt_{i,r}[Q limbs] sigma_{g_r}(c0)   (l limbs)      per giant step, HLINTRANS's MUL /
//                                                       MAC_ADD stages with every buffer and stage key carrying _Grp<i>; pt_{i,r} = pt<(i-1)R+r>
//   v_i = (U_i + ModDown(S_{i,0}), ModDown(S_{i,1}))    modDown(.., "_Grp<i>") and an ADD: G intermediate ciphertexts at level l
//   out = hrotsum(v_1 .. v_G)                           HROTSUM's body with elements h_i, ModUps and stages suffixed _Giant<i>, keys IP_Giant<i>_Key<k>_<j>
//                                                       (stream seed + 10000 + 100000 (16 + i))
// Every sum is formed by the element-wise chains of HLINTRANS and HROTSUM: bit-identical to G hlintrans ops on ct1 (op i with the plaintexts pt_{i,.})
// followed by one hrotsum of their outputs with galois = h.  Unfused, the stages run one launch each; fused, pass (6m) of Arch::fusePasses
// (Planner.cpp) turns the baby key products and the G weighted sums into one launch and pass (6s) the giant step into another.
// identity = 1 adds the identity steps on both axes (below).  Not built: carrying S_{i,0} to the end on the extended basis, a rescale, the sharded plan.
HBSGS::HBSGS(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HBSGS", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  const std::vector<uint32_t> gs = hoistedRotations("hbsgs");
  const uint32_t R = (uint32_t)gs.size(), G = cfg->getValueOr("giants", 4), twoN = 2 * N;
  if (G < 1 || G > 16) throw std::runtime_error("hbsgs: giants = " + S(G) + ", must be in [1, 16]");
  // identity = 1: giant groups i = 0..G and baby steps r = 0..R with g_0 = h_0 = 1.  Group i's identity baby step is the
  // plaintext pt0_<i> (stream seed + 4300 + 100000 i), group 0's rotations are ptg<r> (seed + 4600 + 100000 r).  Group 0 is never brought
  // down on its own: its sums join the giant step's in front of the one final ModDown.  16 terms per accumulator at most
  const bool identity = identityStep("hbsgs"), rescale = rescaleKey("hbsgs");   // rescale: behind the final ModDown only, never the inner groups
  if (identity && R > 15) throw std::runtime_error("hbsgs: rotations = " + S(R) + " with identity = 1, must be in [1, 15]");
  if (identity && G > 15) throw std::runtime_error("hbsgs: giants = " + S(G) + " with identity = 1, must be in [1, 15]");
  const uint32_t gNext = (uint32_t)((uint64_t)gs.back() * cfg->getValueOr("galois", 5) % twoN);
  const uint32_t h = cfg->getValueOr("galois_giant", identity ? gNext : gs.back());   // default g^R mod 2N; with the identity step g^(R+1)
  if (!(h & 1) || h >= twoN) throw std::runtime_error("hbsgs: galois_giant = " + S(h) + " must be odd and below 2N = " + S(twoN));
  std::vector<uint32_t> hs;
  uint64_t hi = 1;
  for (uint32_t i = 1; i <= G; ++i) {
    hi = hi * h % twoN;
    if (std::find(hs.begin(), hs.end(), (uint32_t)hi) != hs.end())
      throw std::runtime_error("hbsgs: galois_giant^" + S(i) + " mod 2N repeats an element: the " + S(G) + " giant steps are not distinct");
    hs.push_back((uint32_t)hi);
  }
  NamedStreams named;
  for (uint32_t i = 0; identity && i <= G; ++i) named.push_back({"pt0_" + S(i), 4300 + 100000ull * i});
  for (uint32_t r = 1; identity && r <= R; ++r) named.push_back({"ptg" + S(r), 4600 + 100000ull * r});
  makeInputs(1, /*plaintext=*/false, /*extPlaintexts=*/G * R, named);

  KeySwitch ks(labelName, maxLevel, currentLevel, alpha, &Datapool, &DataInsMap, &insgener, addrManager.get());
  // the baby step: one ModUp, one key product and one rotated c0 per baby rotation
  const KeySwitch::Digits digits = ks.modUp(cts[0].getC1Addr(), /*inputMayBeOpInput=*/true);
  dispatch(ks.takeStages());
  std::array<std::vector<Limbs>, 3> terms;   // per baby rotation: acc_{r,0}, acc_{r,1}, sigma_r(c0)
  for (uint32_t r = 1; r <= R; ++r) {
    const std::string rs = "_Rot" + S(r);
    const KeySwitch::Accumulators acc = ks.keyProduct(ks.rotateDigits(digits, gs[r - 1], rs), seed + 10000 + 100000ull * r, rs);
    dispatch(ks.takeStages());
    terms[0].push_back(acc[0]); terms[1].push_back(acc[1]); terms[2].push_back(rotateComponent(0, gs[r - 1], rs));
  }
  // per giant step i: HLINTRANS's three weighted sums, the ModDown and the ADD of U_i give v_i
  std::vector<SwitchedSum> v;
  std::array<Limbs, 3> group0;   // the identity step: S_{0,0}, S_{0,1}, U_0 stay on their bases
  Limbs W0;
  const Limbs c0{cts[0].getC0Addr(), {}}, c1{cts[0].getC1Addr(), {}};
  for (uint32_t i = identity ? 0 : 1; i <= G; ++i) {
    const std::string gp = "_Grp" + S(i);
    std::vector<std::vector<AddrType>> pts;
    for (uint32_t r = 1; r <= R; ++r) pts.push_back(namedInputs.at(i ? "pt" + S((i - 1) * R + r) : "ptg" + S(r)));
    std::array<Limbs, 3> sums;
    if (!identity) {
      for (uint32_t t = 0; t < 3; ++t) sums[t] = weightedSum(t, terms[t], pts, gp);
      v.push_back(sumDown(ks, sums, "HBSGS", "HBSGSInner" + gp + "(0)", gp));
      continue;
    }
    const std::vector<AddrType> &pt0 = namedInputs.at("pt0_" + S(i));
    for (uint32_t t = 0; t < 2; ++t) sums[t] = weightedSum(t, terms[t], pts, gp);
    sums[2] = weightedSum(2, terms[2], pts, gp, &c0, &pt0);
    const Limbs W = weightedSum(3, {}, {}, gp, &c1, &pt0);
    if (i == 0) { group0 = sums; W0 = W; }
    else v.push_back(sumDown(ks, sums, "HBSGS", "HBSGSInner" + gp + "(0)", gp, &W));
  }
  // the giant step: HROTSUM's running sums over the v_i
  std::array<Limbs, 3> sums;   // T_0, T_1, V so far
  for (uint32_t i = 1; i <= G; ++i) {
    const std::string gt = "_Giant" + S(i);
    const KeySwitch::Digits dg = ks.modUp(v[i - 1].c1, /*inputMayBeOpInput=*/false, gt);
    const KeySwitch::Accumulators acc = ks.keyProduct(ks.rotateDigits(dg, hs[i - 1], gt), seed + 10000 + 100000ull * (16 + i), gt);
    dispatch(ks.takeStages());
    const std::array<Limbs, 3> term = {acc[0], acc[1], rotateLimbs(v[i - 1].c0, 0, hs[i - 1], gt)};
    for (uint32_t t = 0; t < 3; ++t) sums[t] = i == 1 ? term[t] : addTerm(t, sums[t], term[t], "GiantSum", i, i == G && !identity);
  }
  // the group-0 term last, one ADD per tag; W_0 is the c1 addend behind the ModDown
  for (uint32_t t = 0; identity && t < 3; ++t) sums[t] = addTerm(t, sums[t], group0[t], "GiantSum", 0, true);
  setOutput("out", sumDown(ks, sums, "HBSGS", "HBSGSOutput(0)", "", identity ? &W0 : nullptr), rescale);
  finishConstruction();
}

// reference: HADD::HADD :1114-1176
HADD::HADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HADD", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  makeInputs(2);
  for (uint32_t k = 0; k < 2; k++) {
    PerLimb s{labelName + "_HADD_Level(", ")_k(" + S(k) + ")", range(0, currentLevel), alloc("HADDOutput(" + S(k) + ")", currentLevel)};
    s.a = component(0, k);
    s.c = component(1, k);
    driver.dispatchInstructions("HADD_Key(" + S(k) + ")", eweLimbs(&insgener, EWE_ADD, s));
    setOutput("out", k, s.out);
  }
  finishConstruction();
}

// reference: PMULT::PMULT :1460-1523
PMULT::PMULT(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("PMULT", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  // rescale = 1: both products go through Rescale, out at level - 1
  const bool rescale = rescaleKey("pmult");
  if (rescale && arch->backend() == Arch::BACKEND_SIM) throw std::runtime_error("pmult: rescale = 1 on backend = sim is not supported (the reference's pmult has no rescale)");
  if (rescale && arch->world() > 1) throw std::runtime_error("pmult: rescale = 1 with world > 1 is not supported (the sharded plan is not built)");
  makeInputs(1, /*plaintext=*/true);
  std::array<std::vector<AddrType>, 2> prod;
  for (uint32_t k = 0; k < 2; k++) {
    PerLimb s{labelName + "_PMULT_Level(", ")_k(" + S(k) + ")", range(0, currentLevel), alloc("HMult" + S(k) + "Out", currentLevel)};
    s.a = component(0, k);
    s.b = ptx->getC0Addr();
    driver.dispatchInstructions("PMULT_Key(" + S(k) + ")", eweLimbs(&insgener, EWE_MUL, s));
    prod[k] = s.out;
  }
  if (rescale) setRescaledOutput("out", prod);
  else for (uint32_t k = 0; k < 2; k++) setOutput("out", k, prod[k]);
  finishConstruction();
}

// hrescale (build extension): out = (Rescale(ct1.c0), Rescale(ct1.c1)) at level - 1, the two Rescale builders on the op's own
// input ciphertext (no instruction produces it: inputMayBeOpInput, as the hoisted ModUps)
HRESCALE::HRESCALE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HRESCALE", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  if (arch->backend() == Arch::BACKEND_SIM) throw std::runtime_error("hrescale: backend = sim has no such op (the reference rescales only inside hmult)");
  if (arch->world() > 1) throw std::runtime_error("hrescale: world > 1 is not supported (the sharded plan is not built)");
  makeInputs(1);
  setRescaledOutput("out", {component(0, 0), component(0, 1)}, /*inputMayBeOpInput=*/true);
  finishConstruction();
}

// hmodraise (build extension): ModRaise of a level-1 ciphertext to level T (config key raise_to, default maxLevel).  Per
// component k: c = INTT_{q_0}(ct1.c_k limb 0), then for every j < T out limb j = NTT_{q_j}(centre_{q_0}(c) mod q_j); the centring and the reduction
// run inside the forward transform's first pass (liftSrcMod, hm_ntt_lift), so the 2 (T - 1) lifted limb-polys are never stored.  Limb 0 goes through
// the same launch with source = target modulus: the identity, bit for bit.  Two stages, one launch each, at any batch
HMODRAISE::HMODRAISE(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("HMODRAISE", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  if (arch->backend() == Arch::BACKEND_SIM) throw std::runtime_error("hmodraise: backend = sim has no such op (the reference has no op that raises a level)");
  if (arch->world() > 1) throw std::runtime_error("hmodraise: world > 1 is not supported (the sharded plan is not built)");
  if (currentLevel != 1)
    throw std::runtime_error("hmodraise: level " + S(currentLevel) + " is not supported, the input must be at level 1 (the overflow term of several input limbs is not built)");
  const uint32_t T = cfg->getValueOr("raise_to", maxLevel);
  if (T <= currentLevel || T > maxLevel)
    throw std::runtime_error("hmodraise: raise_to = " + S(T) + ", must be above the input's level " + S(currentLevel) + " and at most maxLevel " + S(maxLevel));
  makeInputs(1);
  std::array<std::vector<AddrType>, 2> coeff, out;
  std::vector<INSGROUP> intt, ntt;
  for (uint32_t k = 0; k < 2; k++) {
    coeff[k] = alloc("ModRaiseINTTOut(" + S(k) + ")", 1);
    out[k] = alloc("HMODRAISEOutput(" + S(k) + ")", T);
  }
  INSGROUP none;   // the input is the op's own ciphertext: no instruction produces it
  for (uint32_t k = 0; k < 2; k++)
    intt.push_back(insgener.GenNTT(0, labelName + "_ModRaise_INTT_k(" + S(k) + ")", &none, false, component(0, k)[0], coeff[k][0], 0));
  driver.dispatchInstructions("ModRaise_INTT", intt);
  for (uint32_t k = 0; k < 2; k++)
    for (uint32_t j = 0; j < T; j++) {
      INSGROUP g = insgener.GenNTT(j, labelName + "_ModRaise_NTT_Level(" + S(j) + ")_k(" + S(k) + ")", &intt[k], true, coeff[k][0], out[k][j], j);
      g[0]->liftSrcMod = 0;   // the stored coefficients are reduced by q_0
      ntt.push_back(g);
    }
  driver.dispatchInstructions("ModRaise_NTT", ntt);
  for (uint32_t k = 0; k < 2; k++) setOutput("out", k, out[k]);
  finishConstruction();
}

// reference: PADD::PADD :1625-1680 (upstream adds the plaintext to both components; only c0 takes it)
PADD::PADD(std::string labelName, uint32_t maxLevel, uint32_t currentLevel, uint32_t alpha, Config *cfg, Arch *_arch)
    : OperationBase("PADD", labelName, cfg, _arch, maxLevel, currentLevel, alpha) {
  makeInputs(1, /*plaintext=*/true);
  for (uint32_t k = 0; k < 2; k++) {
    PerLimb s{labelName + "_PADD_Level(", ")_k(" + S(k) + ")", range(0, currentLevel), alloc("PADDOutput(" + S(k) + ")", currentLevel)};
    s.a = component(0, k);
    s.c = ptx->getC0Addr();
    driver.dispatchInstructions("PADD_Key(" + S(k) + ")", eweLimbs(&insgener, k == 0 ? EWE_ADD : EWE_COPY, s));
    setOutput("out", k, s.out);
  }
  finishConstruction();
}

// =====================================================================================================
// continuous execution
// =====================================================================================================
static OperationBase *makeOp(const std::string &o, uint32_t maxLevel, uint32_t level, uint32_t alpha, Config *cfg, Arch *arch) {
  if (o == "hmult") return new HMULT("test_hmult", maxLevel, level, alpha, cfg, arch);
  if (o == "hrotate") return new HROTATE("test_hrotate", maxLevel, level, alpha, cfg, arch);
  if (o == "hadd") return new HADD("test_hadd", maxLevel, level, alpha, cfg, arch);
  if (o == "pmult") return new PMULT("test_pmult", maxLevel, level, alpha, cfg, arch);
  if (o == "padd") return new PADD("test_ADD", maxLevel, level, alpha, cfg, arch);
  if (o == "hrotate_hoisted") return new HROTATE_HOISTED("test_hrotate_hoisted", maxLevel, level, alpha, cfg, arch);
  if (o == "hlintrans") return new HLINTRANS("test_hlintrans", maxLevel, level, alpha, cfg, arch);
  if (o == "hdot") return new HDOT("test_hdot", maxLevel, level, alpha, cfg, arch);
  if (o == "hrotsum") return new HROTSUM("test_hrotsum", maxLevel, level, alpha, cfg, arch);
  if (o == "hbsgs") return new HBSGS("test_hbsgs", maxLevel, level, alpha, cfg, arch);
  if (o == "hrescale") return new HRESCALE("test_hrescale", maxLevel, level, alpha, cfg, arch);
  if (o == "hmodraise") return new HMODRAISE("test_hmodraise", maxLevel, level, alpha, cfg, arch);
  if (o == "hsquare") return new HSQUARE("test_hsquare", maxLevel, level, alpha, cfg, arch);
  if (o == "hlincomb") return new HLINCOMB("test_hlincomb", maxLevel, level, alpha, cfg, arch);
  if (o == "hmlincomb") return new HMLINCOMB("test_hmlincomb", maxLevel, level, alpha, cfg, arch);
  if (o == "hmuladd") return new HMULADD("test_hmuladd", maxLevel, level, alpha, cfg, arch);
  if (o == "hreim") return new HREIM("test_hreim", maxLevel, level, alpha, cfg, arch);
  if (o == "hclincomb") return new HCLINCOMB("test_hclincomb", maxLevel, level, alpha, cfg, arch);
  if (o == "hplincomb") return new HPLINCOMB("test_hplincomb", maxLevel, level, alpha, cfg, arch);
  if (o == "hdotadd") return new HDOTADD("test_hdotadd", maxLevel, level, alpha, cfg, arch);
  throw std::runtime_error("Error operation requirement, please double confirm!");
}

OpChain::OpChain(const std::string &cfgPath, const std::string &opList, uint32_t maxLevel, uint32_t curLevel, uint32_t alpha,
                 const std::map<std::string, uint32_t> &overrides) {
  std::stringstream ss(opList);
  std::string name;
  std::vector<std::string> names;
  while (std::getline(ss, name, ','))
    if (!name.empty()) names.push_back(name);
  uint32_t level = curLevel;
  try {
    for (size_t i = 0; i < names.size(); ++i) {
      name = names[i];
      if (level == 0) throw std::runtime_error("chain: no limbs left for " + name);
      if (name == "hrotate_hoisted" && i + 1 < names.size())
        throw std::runtime_error("chain: hrotate_hoisted has one output ciphertext per rotation and can only be the last op of a chain");
      Config *cfg = new Config(cfgPath);
      cfgs.push_back(cfg);
      cfg->getValue("N");
      for (auto &kv : overrides) cfg->setValue(kv.first, kv.second);
      // every op draws its own second operand; the first op's first operand is the chain input
      cfg->setValue("seed", cfg->getValueOr("seed", 0x484F4D55u) + 31u * (uint32_t)ops.size());
      Arch *arch = new Arch(cfg);
      archs.push_back(arch);
      OperationBase *op = makeOp(name, maxLevel, level, alpha, cfg, arch);
      if (!ops.empty()) op->bindInput("ct1", ops.back());
      ops.push_back(op);
      if (i + 1 < names.size()) level = op->outputLevel();
    }
    if (ops.empty()) throw std::runtime_error("chain: empty op list");
  } catch (...) {
    for (auto *o : ops) delete o;
    for (auto *a : archs) delete a;
    for (auto *c : cfgs) delete c;
    throw;
  }
}
OpChain::~OpChain() {
  for (auto *o : ops) delete o;
  for (auto *a : archs) delete a;
  for (auto *c : cfgs) delete c;
}
void OpChain::prepare() { for (auto *o : ops) o->prepare(); }
void OpChain::run() { for (auto *a : archs) a->run(); }
void OpChain::sync() { for (auto *a : archs) a->sync(); }
double OpChain::execute(uint32_t iters) {
  prepare();
  run();
  sync();
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < iters; ++i) run();
  sync();
  return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (iters ? iters : 1);
}
bool OpChain::simulate() {
  if (!archs.empty() && archs[0]->backend() == Arch::BACKEND_SIM) {  // the reference cannot chain: every op is simulated on its own
    unsigned long long cycles = 0;
    for (size_t i = 0; i < ops.size(); ++i) { ops[i]->simulate(); cycles += archs[i]->getCycle(); }
    std::cout << "\nChain of " << ops.size() << " operations, simulated one by one: " << cycles << " cycles in total\n";
    return true;
  }
  prepare();
  for (auto *o : ops) o->simulate();
  const double ns = execute(20);
  std::cout << "\nChain of " << ops.size() << " operations, ciphertext resident in HBM: " << (unsigned long long)ns << " ns per pass\n";
  return true;
}
