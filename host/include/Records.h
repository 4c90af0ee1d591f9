// Records.h — what a limb-level record (Instruction.h) reads and writes, said ONCE.
// Every fusion pass (host/src/Planner.cpp) and the launch builder (Arch::buildLaunches) ask these functions and filter by role;
// whoever adds an address-carrying field to Instruction adds it here and nowhere else.
#ifndef HOMULATOR_RECORDS_H
#define HOMULATOR_RECORDS_H
#include <algorithm>

#include "Instruction.h"

// operands of operandList[0..3] an EWE opcode reads, as a bit mask (index: ewe_opcode)
inline int eweOperandMask(ewe_opcode op) {
  static const int m[10] = {3, 15, 7, 5, 5, 1, 5, 1, 13, 1};
  return m[op];
}

// a key-product record that runs the forward transform of at least one digit inside the kernel (pass 7: the transform x key form)
inline bool transformsInside(const Instruction &i) { return std::find(i.ipCoeff.begin(), i.ipCoeff.end(), 1) != i.ipCoeff.end(); }
inline bool isKeyProduct(const Instruction &i) { return i.ops == IP && !i.ipX.empty(); }

enum class Role {
  Operand,        // operandList entry of an element-wise op, a forward transform, an automorphism ...
  InttIn,         // the input of an inverse transform
  SecondPassIn,   // ... of one that keeps only its second pass (7b): its own output limb, where the key product left the first pass
  IpDigit,        // key product: a digit read in evaluation form (hoisted: the unrotated digit)
  IpCoeffSrc,     // ... a digit in coefficient form, transformed inside the kernel (ipSrc[j] with ipCoeff[j])
  IpReplacedSrc,  // ... the conversion output ipSrc[j] that the fused conversion ipConvIn[j] replaces: never written, never loaded
  ConvIn,         // input of a base conversion: a BCONV record's own, ipConvIn[j] (digit = j), fConvIn
  Key,            // key product: evaluation-key limb
  LinPlain,       // weighted sums of hoisted key products (6l, 6m): a rotation's plaintext limb, of one sum
  LinAddend,      // ... the addend source, read through every rotation's automorphism (the unrotated c0)
  LinIdPlain,     // ... the identity step: the plaintext limb of the unrotated term, of one sum
  LinAddend1,     // ... and the second addend source it multiplies, read where it is stored (the unrotated c1; c0 is LinAddend)
  SumAddend,      // sum of rotations of different ciphertexts (6s): a ciphertext's addend source, read through its automorphism (its unrotated c0)
  SumInit,        // ... with initial sums: the polynomial S_k starts from
  SumAddendInit,  // ... and the one the addend sum starts from
  Minuend, Addend, Mix,   // fused forward transform (4, 4b)
  MinuendMul,             // ... (4p) the second factor of a minuend that is a product
  InttMul,                // (4p) the second factor of an inverse transform's input that is a product
  LiftIn,                 // the input of a forward transform that lifts it from another modulus (liftSrcMod, ModRaise): not an Operand, so the passes that
                          // fold a producer into a transform's input or read it through an automorphism (9, 12) leave the record alone
  EpiSub, EpiAdd,         // conversion with the element-wise epilogue (10): fSubFrom, fAdd
  ReplacedIn      // the transform input operandList[0] that the fused conversion fConvIn replaces (9): never written, never loaded
};
struct Read {
  AddrType addr;
  Role role;
  size_t digit;   // key product: index into ipX; otherwise kNoDigit
  // what the kernels load: everything but the two "replaced" roles.  The passes that count the readers of an address (6h-10, 12) count
  // those too — the never-written address has this record as its one reader, which is what makes its producer foldable
  bool loaded() const { return role != Role::IpReplacedSrc && role != Role::ReplacedIn; }
};
static const size_t kNoDigit = (size_t)-1;

// Every address the record reads.  The order is part of the contract: the sharded gather plan replicates foreign operands in first-read
// order (Arch::buildLaunches), so a replaced address sits directly in front of the first input of the conversion that replaces it and the
// remaining conversion inputs follow the record's other operands, as the launch builder has always listed them.
inline std::vector<Read> recordReads(const Instruction &i) {
  std::vector<Read> v;
  if (isKeyProduct(i)) {
    const std::vector<AddrType> &src = i.ipSrc.empty() ? i.ipX : i.ipSrc;
    auto converted = [&](size_t j) { return j < i.ipConvIn.size() && !i.ipConvIn[j].empty(); };
    for (size_t j = 0; j < src.size(); ++j) {
      if (converted(j)) { v.push_back({src[j], Role::IpReplacedSrc, j}); v.push_back({i.ipConvIn[j][0], Role::ConvIn, j}); }
      else v.push_back({src[j], j < i.ipCoeff.size() && i.ipCoeff[j] ? Role::IpCoeffSrc : Role::IpDigit, j});
    }
    for (size_t j = 0; j < src.size(); ++j)
      if (converted(j))
        for (size_t x = 1; x < i.ipConvIn[j].size(); ++x) v.push_back({i.ipConvIn[j][x], Role::ConvIn, j});
    for (size_t c = 1; c < i.ipSumX.size(); ++c)   // (6s): the digits of the further ciphertexts, behind the first one's (ipX, above)
      for (size_t j = 0; j < i.ipSumX[c].size(); ++j) v.push_back({i.ipSumX[c][j], Role::IpDigit, j});
    for (auto &y : i.ipY)
      for (AddrType a : y) v.push_back({a, Role::Key, kNoDigit});
    for (auto &row : i.ipLinPt)
      for (AddrType a : row) v.push_back({a, Role::LinPlain, kNoDigit});
    if (i.ipLinAddend) v.push_back({i.ipLinAddend, Role::LinAddend, kNoDigit});
    for (AddrType a : i.ipLinIdPt) v.push_back({a, Role::LinIdPlain, kNoDigit});
    if (i.ipLinAddend1) v.push_back({i.ipLinAddend1, Role::LinAddend1, kNoDigit});
    for (AddrType a : i.ipSumAddend) v.push_back({a, Role::SumAddend, kNoDigit});
    for (AddrType a : i.ipSumInit) v.push_back({a, Role::SumInit, kNoDigit});
    if (i.ipSumAddendInit) v.push_back({i.ipSumAddendInit, Role::SumAddendInit, kNoDigit});
    return v;
  }
  if (i.ops == BCONV_STEP2) {
    for (size_t x = 0; x + 1 < i.operandList.size(); ++x) v.push_back({i.operandList[x], Role::ConvIn, kNoDigit});
  } else if (i.fu.form != FusedForm::None) {   // (5d .. 5a): the form's reads in its own order (Instruction.h), pair 1's (operandList) among them
    for (AddrType a : i.fu.reads) v.push_back({a, Role::Operand, kNoDigit});
  } else if (i.ops == MULT) {
    for (int b = 0; b < 4; ++b)
      if (eweOperandMask(i.opcode) & (1 << b)) v.push_back({i.operandList[b], Role::Operand, kNoDigit});
  } else {
    const Role r = !i.fConvIn.empty() ? Role::ReplacedIn : i.ops == NTT && i.liftSrcMod != kNoLift ? Role::LiftIn : i.ops != INTT ? Role::Operand : i.secondOnly ? Role::SecondPassIn : Role::InttIn;
    v.push_back({i.operandList[0], r, kNoDigit});
    if (!i.fConvIn.empty()) v.push_back({i.fConvIn[0], Role::ConvIn, kNoDigit});
    if (i.inMulB) v.push_back({i.inMulB, Role::InttMul, kNoDigit});
  }
  if (i.fusedSubScale) {
    v.push_back({i.fMinuend, Role::Minuend, kNoDigit});
    if (i.fMinuendB) v.push_back({i.fMinuendB, Role::MinuendMul, kNoDigit});
    if (i.fAddend) v.push_back({i.fAddend, Role::Addend, kNoDigit});
    if (i.fMix) v.push_back({i.fMix, Role::Mix, kNoDigit});
  }
  if (i.ops != BCONV_STEP2 && i.ops != MULT)
    for (size_t x = 1; x < i.fConvIn.size(); ++x) v.push_back({i.fConvIn[x], Role::ConvIn, kNoDigit});
  if (i.fusedEpi) {
    v.push_back({i.fSubFrom, Role::EpiSub, kNoDigit});
    if (i.fAdd) v.push_back({i.fAdd, Role::EpiAdd, kNoDigit});
  }
  return v;
}

enum class WriteRole { Output, Scratch };   // Scratch: ipX[j] of a digit transformed inside the key product, the hand-off of its first pass
struct Write { AddrType addr; WriteRole role; };
inline std::vector<Write> recordWrites(const Instruction &i) {
  std::vector<Write> v = {{i.OutputOperand, WriteRole::Output}};
  for (AddrType o : i.extraOutputs) v.push_back({o, WriteRole::Output});
  for (size_t j = 0; j < i.ipCoeff.size(); ++j)
    if (i.ipCoeff[j]) v.push_back({i.ipX[j], WriteRole::Scratch});
  return v;
}
#endif
