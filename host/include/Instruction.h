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
  bool sumHead = false;      // a tensor product's MAC2 (d1) that is pair 1 of a SUM of tensor products (HDOT): pass (5d) starts its record here
  bool squareHead = false;   // a tensor product's MAC2 (d1) of a ciphertext with ITSELF (HSQUARE): pass (5q) starts its record here
  bool lincombHead = false;  // the MUL_CONST of term 1 of a sum of scaled ciphertexts (HLINCOMB): pass (5l) starts its record here
  bool muladdHead = false;   // a tensor product's MAC2 (d1) that scalars, scaled addends and a constant follow (HMULADD): pass (5m) starts its record here
  bool reimHead = false;     // the ADD x + conj(x) of one limb and component (HREIM): pass (5r) starts its record here
  bool clincombHead = false; // the MUL_CONST a_1 x_1 of term 1 of a complex-weighted sum of ciphertexts (HCLINCOMB): pass (5c) starts its record here
  bool plincombHead = false; // the MUL p_1 x_1 of term 1 of one component of a plaintext-weighted sum of ciphertexts (HPLINCOMB): pass (5p) starts its record here;
                             // also the ADD of that sum's plaintext addend, which the pass takes behind the last term only if it is marked
  bool dotaddHead = false;   // a tensor product's MAC2 (d1) that is pair 1 of a scaled SUM of tensor products plus scaled addends plus a constant (HDOTADD):
                             // pass (5a) starts its record here
  std::vector<uint32_t> inMods;  // BCONV: modulus ids of the inputs
  unsigned long long refInstructions = 0;  // upstream instructions this record stands for
  unsigned long long refExtra = 0;         // ... of records folded into a BCONV record (not scaled by its MAC-port count)
  // set by the backend's fusion passes (Arch::fusePasses, host/src/Planner.cpp), never by the generators; the fields that hold addresses
  // are listed ONCE more, with their roles, in recordReads / recordWrites (Records.h): add a new one there too
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
  // (5d) sum of tensor products (hm_tensor_dot): a fusedTensor record that absorbed the chains behind its three outputs.  dotOperands = (c00, c10,
  // c01, c11) of every pair, pair 1 first; OutputOperand = the final d1, extraOutputs = the final d0, d2.  Empty: a plain tensor product
  std::vector<AddrType> dotOperands;
  // (5q) scaled square plus constant (hm_tensor_square): a fusedTensor record of a ciphertext with itself.  sqOperands = (c0, c1): its two reads;
  // OutputOperand = the final d1, extraOutputs = the final d0, d2.  sqHasScale: the MUL_CONST records behind its three outputs went in, all
  // with the constant sqScale; sqHasConst: the ADD_CONST record behind d0 went in, with the constant sqConst.  sqOperands empty: not a square
  std::vector<AddrType> sqOperands;
  bool sqHasScale = false, sqHasConst = false;
  uint64_t sqScale = 1, sqConst = 0;
  // (5l) sum of scaled polynomials plus constant (hm_lincomb): the MUL_CONST record of term 1 that absorbed the MUL_CONST + ADD pairs of the further
  // terms and the ADD_CONST behind them.  lcOperands = the T inputs in term order, lcScales = their scalars; OutputOperand = the final sum.
  // lcHasConst: the ADD_CONST record went in, with the constant lcConst.  lcOperands empty: not such a sum
  std::vector<AddrType> lcOperands;
  std::vector<uint64_t> lcScales;
  bool lcHasConst = false;
  uint64_t lcConst = 0;
  // (5L) several (5l) sums over ONE list of inputs (hm_lincomb_multi): the first of them, which absorbed the others.  lcOperands = the shared T
  // inputs; mlScales[m] = the T scalars of output m, mlConsts[m] = its constant (0 where the absorbed record had none; mlHasConst: some had
  // one); OutputOperand = output 1, extraOutputs = outputs 2 .. M, in the order the sums were emitted.  mlScales empty: not such a record
  std::vector<std::vector<uint64_t>> mlScales;
  std::vector<uint64_t> mlConsts;
  bool mlHasConst = false;
  // (5m) scaled tensor product plus scaled addends plus constant (hm_tensor_muladd): a fusedTensor record that absorbed the chains behind its
  // outputs.  maOperands = (c00, c10, c01, c11) of the product, then (x_t, y_t) of every addend; maAddScales = the scalars u_t; OutputOperand = the
  // final d1, extraOutputs = the final d0, d2.  maHasScale: the MUL_CONST records behind the three outputs went in, all with the constant
  // maScale; maHasConst: the ADD_CONST record behind d0 went in, with the constant maConst.  maOperands empty: not such a record
  std::vector<AddrType> maOperands;
  std::vector<uint64_t> maAddScales;
  bool maHasScale = false, maHasConst = false;
  uint64_t maScale = 1, maConst = 0;
  // (5r) real and imaginary parts from a polynomial and its conjugate (hm_reim_split): the ADD record x + y that absorbed the SUB x - y of the same
  // operands and the MUL of the difference by the evaluation form of -X^(N/2).  reimOperands = (x, y): its two reads; OutputOperand = the sum,
  // extraOutputs = the product.  The stored factor is not read: the kernel derives it.  reimOperands empty: not such a record
  std::vector<AddrType> reimOperands;
  // (5c) sum of polynomials times a + b X^(N/2) plus constant (hm_clincomb): the MUL_CONST record a_1 x_1 of term 1 that absorbed, per term, the
  // MUL by the stored monomial, its MUL_CONST, the ADD of both parts and the ADD onto the running sum, and the ADD_CONST behind them.
  // clOperands = the T inputs in term order, clScalesRe = a_t, clScalesIm = b_t (the stages carry q - b_t: the stored monomial is -X^(N/2));
  // OutputOperand = the final sum.  clHasConst: the ADD_CONST record went in, with the constant clConst.  The stored monomial is not read: the
  // kernel derives it.  clOperands empty: not such a sum
  std::vector<AddrType> clOperands;
  std::vector<uint64_t> clScalesRe, clScalesIm;
  bool clHasConst = false;
  uint64_t clConst = 0;
  // (5p) sum of ciphertexts times plaintexts plus a plaintext on c0 (hm_plincomb): the MUL record p_1 x_1 of c0's chain that absorbed the MAC_ADD
  // records behind it, the ADD of the addend, and the whole chain of c1 on the same plaintext limbs.  plOperands = (p_t, x_t, y_t) per term, in
  // term order; plAddend = the plaintext limb added to c0 (plHasAddend); OutputOperand = c0's final sum, extraOutputs = c1's.  plOperands empty:
  // not such a sum
  std::vector<AddrType> plOperands;
  bool plHasAddend = false;
  AddrType plAddend = 0;
  // (5a) scaled sum of tensor products plus scaled addends plus constant (hm_tensor_dotadd): a fusedTensor record that absorbed the tensor records
  // of the further pairs and the chains behind the outputs.  daOperands = (c00, c10, c01, c11) of every pair, pair 1 first, then (x_r, y_r) of
  // every addend; daScales = the scalar s_t of every pair (1: the pair had no MUL_CONST records), daAddScales = the scalars u_r; OutputOperand =
  // the final d1, extraOutputs = the final d0, d2.  daHasScale: the MUL_CONST records of at least one pair went in; daHasConst: the ADD_CONST
  // record behind d0 went in, with the constant daConst.  daOperands empty: not such a record
  std::vector<AddrType> daOperands;
  std::vector<uint64_t> daScales, daAddScales;
  bool daHasScale = false, daHasConst = false;
  uint64_t daConst = 0;
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
