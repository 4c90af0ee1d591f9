// Instruction.h — one LIMB-level operation of a stage.
// The reference's Instruction (include/Instruction.h:26-188) is one 256-coefficient batch of one limb and
// carries only address tokens and an op kind; a GPU launch covers a whole stage, so this build's record is
// per limb, stands for `refInstructions` upstream instructions (batchCount of them; x InLevel for BCONV),
// and carries what the timing model lacks: modulus id, EWE opcode, constants, Galois element, input basis.
#ifndef HOMULATOR_INSTRUCTION_H
#define HOMULATOR_INSTRUCTION_H
#include "Basic.h"

enum ins_ops { NTT, INTT, MULT, MADD, MSUB, BCONV_STEP1, BCONV_STEP2, AUTO, DS, PRNG, IP, FETCH_RF, STORE_RF };
extern std::vector<std::string> ins_ops_name;

// the arithmetic of an EWE ("MULT"-tagged) instruction; numbering = include/homulator_hip.h hm_ewe_op
enum ewe_opcode {
  EWE_MUL = 0, EWE_MAC2 = 1, EWE_MAC_ADD = 2, EWE_ADD = 3, EWE_SUB = 4,
  EWE_MUL_CONST = 5, EWE_SUB_SCALE = 6, EWE_COPY = 7, EWE_SUB_SCALE_ADD = 8, EWE_ADD_CONST = 9
};

static const uint32_t kNoLift = 0xFFFFFFFFu;   // Instruction::liftSrcMod of a plain forward transform

// The fused element-wise records of passes (5d) .. (5a) (host/src/Planner.cpp): which kernel family a record has become (Fused::form), and, as
// Instruction::mark, which pass the op builder wants to start at a record.  The marks, per form:
//   TensorDot     a tensor product's MAC2 (d1) that is pair 1 of a SUM of tensor products (HDOT): pass (5d)
//   Square        a tensor product's MAC2 (d1) of a ciphertext with ITSELF (HSQUARE): pass (5q)
//   Lincomb       the MUL_CONST of term 1 of a sum of scaled ciphertexts (HLINCOMB, HMLINCOMB): pass (5l)
//   LincombMulti  (never a mark: pass (5L) merges the records (5l) formed)
//   MulAdd        a tensor product's MAC2 (d1) that scalars, scaled addends and a constant follow (HMULADD): pass (5m)
//   ReIm          the ADD x + conj(x) of one limb and component (HREIM): pass (5r)
//   CLincomb      the MUL_CONST a_1 x_1 of term 1 of a complex-weighted sum of ciphertexts (HCLINCOMB): pass (5c)
//   PLincomb      the MUL p_1 x_1 of term 1 of one component of a plaintext-weighted sum of ciphertexts (HPLINCOMB): pass (5p); also the ADD of
//                 that sum's plaintext addend, which the pass takes behind the last term only if it is marked
//   DotAdd        a tensor product's MAC2 (d1) that is pair 1 of a scaled SUM of tensor products plus scaled addends plus a constant (HDOTADD):
//                 pass (5a)
enum class FusedForm : uint8_t { None, TensorDot, Square, Lincomb, LincombMulti, MulAdd, ReIm, CLincomb, PLincomb, DotAdd };

// What a fused element-wise record reads and carries, whatever its form.  `reads` is every address it reads, in the order recordReads
// (Records.h) reports them; the outputs are the record's OutputOperand and extraOutputs.  Per form (T = terms, A = addends):
//   TensorDot (hm_tensor_dot)        a fusedTensor record that absorbed the chains behind its three outputs.  reads = (c00, c10, c01, c11) of
//                                    every pair, pair 1 first; OutputOperand = the final d1, extraOutputs = the final d0, d2
//   Square (hm_tensor_square)        a fusedTensor record of a ciphertext with itself.  reads = (c0, c1); outputs as TensorDot.  hasScale: the
//                                    MUL_CONST records behind its three outputs went in, all with the constant scales[0]; hasConst: the ADD_CONST
//                                    record behind d0 went in, with `constant`
//   Lincomb (hm_lincomb)             the MUL_CONST record of term 1 that absorbed the MUL_CONST + ADD pairs of the further terms and the ADD_CONST
//                                    behind them.  reads = the T inputs in term order, scales = their scalars; OutputOperand = the final sum;
//                                    hasConst / constant: the ADD_CONST record
//   LincombMulti (hm_lincomb_multi)  several Lincomb records over ONE list of inputs: the first of them, which absorbed the others.  reads = the
//                                    shared T inputs; rowScales[m] = the T scalars of output m, rowConsts[m] = its constant (0 where the absorbed
//                                    record had none; hasConst: some had one); OutputOperand = output 1, extraOutputs = outputs 2 .. M, in the
//                                    order the sums were emitted (scales / constant stay output 1's, unread)
//   MulAdd (hm_tensor_muladd)        a fusedTensor record that absorbed the chains behind its outputs.  reads = (c00, c10, c01, c11) of the
//                                    product, then (x_t, y_t) of every addend; scales2 = the scalars u_t; outputs as TensorDot.  hasScale /
//                                    scales[0], hasConst / constant: as Square
//   ReIm (hm_reim_split)             the ADD record x + y that absorbed the SUB x - y of the same operands and the MUL of the difference by the
//                                    evaluation form of -X^(N/2).  reads = (x, y); OutputOperand = the sum, extraOutputs = the product.  The
//                                    stored factor is not read: the kernel derives it
//   CLincomb (hm_clincomb)           the MUL_CONST record a_1 x_1 of term 1 that absorbed, per term, the MUL by the stored monomial, its
//                                    MUL_CONST, the ADD of both parts and the ADD onto the running sum, and the ADD_CONST behind them.  reads = the
//                                    T inputs in term order, scales = a_t, scales2 = b_t (the stages carry q - b_t: the stored monomial is
//                                    -X^(N/2), which is not read); OutputOperand = the final sum; hasConst / constant: the ADD_CONST record
//   PLincomb (hm_plincomb)           the MUL record p_1 x_1 of c0's chain that absorbed the MAC_ADD records behind it, the ADD of the addend, and
//                                    the whole chain of c1 on the same plaintext limbs.  reads = (p_t, x_t, y_t) per term, in term order, then,
//                                    with hasAddend, the plaintext limb added to c0; OutputOperand = c0's final sum, extraOutputs = c1's
//   DotAdd (hm_tensor_dotadd)        a fusedTensor record that absorbed the tensor records of the further pairs and the chains behind the outputs.
//                                    reads = (c00, c10, c01, c11) of every pair, pair 1 first, then (x_r, y_r) of every addend; scales = the
//                                    scalar s_t of every pair (1: the pair had no MUL_CONST records), scales2 = the scalars u_r; outputs as
//                                    TensorDot.  hasScale: the MUL_CONST records of at least one pair went in; hasConst / constant: as Square
struct Fused {
  FusedForm form = FusedForm::None;
  std::vector<AddrType> reads;
  uint32_t terms = 0, addends = 0;
  std::vector<uint64_t> scales, scales2;
  std::vector<std::vector<uint64_t>> rowScales;
  std::vector<uint64_t> rowConsts;
  bool hasScale = false, hasConst = false, hasAddend = false;
  uint64_t constant = 0;
};

class Instruction {
public:
  ins_ops ops;
  std::string Name;
  uint32_t level_id = 0;   // limb index inside its buffer (reference: level_id)
  uint32_t mod_id = 0;     // modulus id (q_i: i, p_j: maxLevel + j)
  std::vector<AddrType> operandList;  // up to 4 operands (0 = "fake operand", src/mem.cpp:30); BCONV: the inputs
  AddrType OutputOperand = 0;
  ewe_opcode opcode = EWE_MUL;
  bool hasConstant = false;
  uint64_t constant = 0;   // per-limb constant of MUL_CONST / SUB_SCALE, or the INTT epilogue scale
  uint32_t galois = 0;
  bool passthrough = false;  // an NTT-kind instruction whose input is already in evaluation form (copy)
  FusedForm mark = FusedForm::None;   // set by the op builder: the pass of this form starts its record here (see FusedForm); at most one per record
  std::vector<uint32_t> inMods;  // BCONV: modulus ids of the inputs
  unsigned long long refInstructions = 0;  // upstream instructions this record stands for
  unsigned long long refExtra = 0;         // ... of records folded into a BCONV record (not scaled by its MAC-port count)
  // set by the backend's fusion passes (Arch::fusePasses, host/src/Planner.cpp), never by the generators; the fields that hold addresses
  // are listed ONCE more, with their roles, in recordReads / recordWrites (Records.h): add a new one there too.  (A new fused element-wise
  // form needs no field: it is one more FusedForm, whose reads are Fused::reads)
  bool fusedSubScale = false;          // forward NTT whose epilogue is out = (minuend - NTT(in)) * constant [+ addend]
  AddrType fMinuend = 0, fAddend = 0;  // fAddend == 0: no addend
  // merged ModDown + rescale: the transform's input is in + fMixConst * fMix, the addend is scaled by fAddendConst
  AddrType fMix = 0;                   // 0: no prologue
  uint64_t fMixConst = 0, fAddendConst = 0;  // fAddendConst == 0: addend as is
  // (9) the transform's input operandList[0] is this base conversion, computed inside the transform's first pass (never written)
  std::vector<AddrType> fConvIn;
  std::vector<uint32_t> fConvMods;     // ... its input moduli
  // (10) a BCONV_STEP2 record with the element-wise epilogue out = (fSubFrom - conv) * constant [+ fAdd] (the rescale residue of 4c)
  bool ipInvOut = false;     // IP record (7b, round 5): its outputs leave the kernel as the first pass of their inverse transform
  bool secondOnly = false;   // INTT record (7b): the first pass has been run into its output limb by the producing IP record
  bool packedOut = false;    // INTT record (11, round 5): the output is stored in the split-30 packed form (only base conversions read it)
  bool inPacked = false;     // BCONV record / fused transform with fConvIn (11): the conversion's inputs are stored packed
  std::vector<uint8_t> ipConvPacked;   // IP record (11): per digit, the inputs of the digit's fused conversion are stored packed
  // (12, round 6) an AUTO record folded into its readers: an INTT record reads its input, a fused forward transform its addend, through X -> X^g
  uint32_t inGalois = 0, fAddendGalois = 0;   // 0: as stored
  uint32_t ipXGalois = 0;                     // ... and a transform x key record its evaluation-form digits (hm_ntt_ip_desc.x_galois)
  // (4p) product operands of transforms: an EWE_MUL of two op inputs folded into its one reader.  A fused forward transform's minuend is
  // fMinuend * fMinuendB, an INTT record's input operandList[0] * inMulB.  0: a plain operand
  AddrType fMinuendB = 0, inMulB = 0;
  // (ModRaise, HMODRAISE) a forward transform whose stored input is reduced by ANOTHER modulus, liftSrcMod: the transform centres it against that
  // modulus and reduces it into its own (mod_id) while it loads.  Set by the op builder, read by the launch builder.  kNoLift: a plain input
  uint32_t liftSrcMod = kNoLift;
  bool fusedEpi = false;
  AddrType fSubFrom = 0, fAdd = 0;
  bool fusedTensor = false;            // MAC2 record that also produces d0 -> extraOutputs[0] and d2 -> extraOutputs[1]
  std::vector<AddrType> extraOutputs;
  Fused fu;                            // (5d .. 5a) the fused element-wise record this one has become; fu.form == None: none of them
  // fused inner product (ops == IP): out_k = sum_j ipX[j] * ipY[k][j]; out_0 = OutputOperand, out_1 = extraOutputs[0]
  std::vector<AddrType> ipX;
  std::vector<std::vector<AddrType>> ipY;
  // fused NTT-epilogue x key MAC (Planner.cpp pass (7)): digit j with ipCoeff[j] set is still in coefficient
  // form at ipSrc[j] and goes through the forward transform inside the inner-product kernel; ipX[j] (the buffer the separate
  // transform would have written: NTTOut_beta(j)) then only serves as the scratch of its first pass
  std::vector<AddrType> ipSrc;
  std::vector<uint8_t> ipCoeff;
  // (8) the base conversion that produces such a digit moves into the transform's first pass as well: ipConvIn[j] = the conversion's
  // input limbs, ipConvMods[j] their moduli (empty: digit j is not converted inside the kernel)
  std::vector<std::vector<AddrType>> ipConvIn;
  std::vector<std::vector<uint32_t>> ipConvMods;
  // (6h) hoisted key product (hm_inner_product_hoisted): ipX = the UNROTATED digits, rotation r reads them through X -> X^ipHoistG[r] with keys
  // ipY[2r + k]; its outputs are out_{r,k} = (OutputOperand, extraOutputs...)[2r + k].  Empty: not hoisted
  std::vector<uint32_t> ipHoistG;
  // (6m, 6l) M weighted sums of the hoisted key products (M = 1: hm_inner_product_lintrans, M >= 2: hm_inner_product_lintrans_multi): a hoisted
  // record (ipX, ipY, ipHoistG as above) whose rotation r is multiplied by the plaintext limb ipLinPt[m][r] and summed over r before it is stored.
  // ipLinAddend != 0 (the Q limbs): U_m = sum_r ipLinPt[m][r] * sigma_r(ipLinAddend) as well.  With w = 2 + (ipLinAddend != 0) outputs per sum,
  // (OutputOperand, extraOutputs...)[m * w + k] = S_{m,k}, k < 2, and [m * w + 2] = U_m.  ipLinPt empty: no weighted sum
  std::vector<std::vector<AddrType>> ipLinPt;
  AddrType ipLinAddend = 0;
  // ... with the identity step (hm_inner_product_lintrans_id; the Q limbs, with ipLinAddend): U_m also takes ipLinIdPt[m] * ipLinAddend, unrotated,
  // and W_m = ipLinIdPt[m] * ipLinAddend1 (the unrotated c1) is one more output: w = 4 and [m * w + 3] = W_m.  ipLinIdPt empty: no identity step
  std::vector<AddrType> ipLinIdPt;
  AddrType ipLinAddend1 = 0;
  // (6s) sum of the key products of rotations of DIFFERENT ciphertexts (hm_inner_product_rotsum): ciphertext c reads its own unrotated digits
  // ipSumX[c] (ipSumX[0] == ipX) through X -> X^ipHoistG[c] with keys ipY[2c + k], and the sum over c is formed before it is stored:
  // OutputOperand = S_0, extraOutputs[0] = S_1.  ipSumAddend non-empty (the Q limbs): extraOutputs[1] = sum_c sigma_c(ipSumAddend[c]).
  // ipSumX empty: no such sum
  std::vector<std::vector<AddrType>> ipSumX;
  std::vector<AddrType> ipSumAddend;
  // ... with initial sums (hm_inner_product_rotsum_init): S_k starts from ipSumInit[k] and, with ipSumAddend, the addend sum from
  // ipSumAddendInit, each read where the outputs are written.  ipSumInit empty: the sums start from zero
  std::vector<AddrType> ipSumInit;
  AddrType ipSumAddendInit = 0;
  std::vector<Instruction *> depsInsList;

  Instruction(std::string name, ins_ops op, uint32_t level) : ops(op), Name(std::move(name)), level_id(level) {}
  const std::string &GetOpName() const { return ins_ops_name[ops]; }
  const std::string &GetName() const { return Name; }
  uint32_t getinputCount() const { return (uint32_t)operandList.size(); }
  AddrType getOperand(uint32_t i) const { return operandList[i]; }
};

typedef std::vector<Instruction *> INSGROUP;
#endif
