// Planner.cpp — the fusion passes on the stage list (fuse = 1): Arch::fusePasses is the list of passes, each pass a function of its own.
// All of them preserve every value that a later stage or the caller can observe except the intermediates they eliminate (listed in
// DESIGN.md §5).  What a record reads and writes is asked of Records.h; a pass that needs "who reads this address" filters recordReads().
#include <algorithm>
#include <array>
#include <iterator>
#include <set>

#include "Arch.h"
#include "Records.h"
#include "../../homulator_amd/csrc/hm_params.h"
#include "../../include/homulator_hip.h"

struct Arch::Planner {
  Arch &A;
  std::vector<Stage> &st;
  // consumers of every address, counted ONCE, before pass 1 rewrites operands through its aliases, and never updated: passes 2-6 rely on
  // that snapshot (an address with one consumer then has at most one now).  Passes 6h-12 rebuild their view (readers()) at their own start.
  std::map<AddrType, int> uses;
  // the record that writes an address.  Updated by the passes that move an output (2, 4, 4c, 6, 6h, 10), deliberately not by the others.
  std::map<AddrType, Instruction *> producer;
  std::set<Instruction *> dead;   // (looked up only: nothing may iterate it, a plan must not depend on pointer order)

  Planner(Arch &a, std::vector<Stage> &s) : A(a), st(s) {
    for (auto &s : st)
      for (Instruction *i : s.ins) {
        for (const Read &r : recordReads(*i)) uses[r.addr]++;
        producer[i->OutputOperand] = i;
      }
  }
  bool live(Instruction *i) const { return !dead.count(i); }
  Instruction *producerOf(AddrType a) const { auto p = producer.find(a); return p == producer.end() ? nullptr : p->second; }
  uint32_t cap(const char *name) const { return Arch::cap(A.logN, name); }
  unsigned long long bconvPorts() const { return (unsigned long long)A.config->getValueOr("bconv_num_high", 1) * A.config->getValueOr("bconv_num_width", 1); }
  // every read of every live record, as the record list stands now.  The replaced inputs of fused conversions count (Read::loaded)
  typedef std::map<AddrType, std::vector<Instruction *>> Readers;
  Readers readers() const {
    Readers rd;
    for (auto &s : st)
      for (Instruction *i : s.ins)
        if (live(i))
          for (const Read &r : recordReads(*i)) rd[r.addr].push_back(i);
    return rd;
  }
  static bool onlyReader(Readers &rd, AddrType a, Instruction *i) { auto &v = rd[a]; return v.size() == 1 && v[0] == i; }
  // the one live reader of `a`, if it is an element-wise record of this opcode and modulus (and no tensor record)
  Instruction *soleReader(Readers &rd, AddrType a, ewe_opcode op, uint32_t mod) const {
    auto &r = rd[a];
    return r.size() == 1 && live(r[0]) && r[0]->ops == MULT && r[0]->opcode == op && r[0]->mod_id == mod && !r[0]->fusedTensor ? r[0] : nullptr;
  }
  bool isMul(Instruction *i, uint32_t mod) const { return live(i) && i->ops == MULT && i->opcode == EWE_MUL && i->mod_id == mod; }
  // the `length` records of the chain that starts with `first` (a MUL) and goes on through MAC_ADD records of its modulus, each the only reader
  // of the one before, which is its operand c (empty: there is no such chain)
  typedef std::vector<Instruction *> Chain;
  Chain chainFrom(Readers &rd, Instruction *first, size_t length) const {
    Chain c = {first};
    while (c.size() < length) {
      Instruction *next = soleReader(rd, c.back()->OutputOperand, EWE_MAC_ADD, first->mod_id);
      if (!next || next->operandList[2] != c.back()->OutputOperand) return Chain();
      c.push_back(next);
    }
    return c;
  }
  // record `i` goes into `carrier`: it is never run, its upstream instructions are accounted for there
  void absorb(Instruction *carrier, Instruction *i) {
    if (i == carrier || !live(i)) return;
    carrier->refInstructions += i->refInstructions;
    dead.insert(i);
  }
  // the merged key product over rotations that `c` carries (6m/6l, 6s, 6h): digits, keys [2r + k], the rotations' elements, and its outputs
  void carry(Instruction *c, const std::vector<AddrType> &x, const std::vector<std::vector<AddrType>> &ys, const std::vector<uint32_t> &gs,
             const std::vector<AddrType> &outs) {
    c->ipX = x;
    c->ipY = ys;
    c->ipHoistG = gs;
    c->OutputOperand = outs[0];
    c->extraOutputs.assign(outs.begin() + 1, outs.end());
    for (const Write &w : recordWrites(*c)) producer[w.addr] = c;
  }
  // where every record stands, (stage, position), as the stages are when a pass starts: a record that absorbed later ones moves to the place of
  // the last of them (5d, 6s)
  struct Placement {
    std::vector<Stage> &st;
    std::map<Instruction *, std::pair<size_t, size_t>> at;
    explicit Placement(std::vector<Stage> &stages) : st(stages) {
      for (size_t si = 0; si < st.size(); ++si)
        for (size_t k = 0; k < st[si].ins.size(); ++k) at[st[si].ins[k]] = {si, k};
    }
    bool after(Instruction *a, Instruction *b) { return at[a] > at[b]; }
    void moveTo(Instruction *carrier, Instruction *last) {
      if (last == carrier) return;
      auto &from = st[at[carrier].first].ins;
      from.erase(std::remove(from.begin(), from.end(), carrier), from.end());
      auto &to = st[at[last].first].ins;
      std::replace(to.begin(), to.end(), last, carrier);
    }
  };

  // ---- what the passes (5d) .. (5a) share: the marked records, the links they follow, and the record that absorbs them
  // the live records the op builder marked for the pass of `form` (Instruction::mark) and that no pass has taken, in stage order
  std::vector<Instruction *> markedHeads(FusedForm form) const {
    std::vector<Instruction *> heads;
    for (auto &s : st)
      for (Instruction *i : s.ins)
        if (live(i) && i->mark == form && i->fu.form == FusedForm::None) heads.push_back(i);
    return heads;
  }
  bool isScaled(Instruction *i, uint32_t mod) const { return i->ops == MULT && i->opcode == EWE_MUL_CONST && i->hasConstant && i->mod_id == mod; }
  // a tensor record's MAC2 operands are (P, S, R, T) = (c00, c11, c01, c10); the forms list a pair as (c00, c10, c01, c11)
  static std::vector<AddrType> pairOperands(const Instruction *i) { return {i->operandList[0], i->operandList[3], i->operandList[2], i->operandList[1]}; }
  typedef std::array<AddrType, 3> Triple;        // d0, d1, d2 of a tensor form
  typedef std::array<Instruction *, 3> Three;
  static Triple tensorOutputs(const Instruction *i) { return {i->extraOutputs[0], i->OutputOperand, i->extraOutputs[1]}; }
  // the MUL_CONST records that are the only readers of the three polynomials `of`, if all three carry one constant
  bool scalars(Readers &rd, const Triple &of, uint32_t mod, Three &m) const {
    for (int i = 0; i < 3; ++i) m[i] = soleReader(rd, of[i], EWE_MUL_CONST, mod);
    return m[0] && m[1] && m[2] && m[0]->hasConstant && m[1]->hasConstant && m[2]->hasConstant && m[0]->constant == m[1]->constant &&
           m[0]->constant == m[2]->constant;
  }
  // the ADD behind `sum` if that is all that reads it, and its other operand.  eitherSide: the sum may be either operand of the ADD ((5l), (5m),
  // (5a)); otherwise only its operand a ((5c), (5p): their builders emit it there, and the passes have never taken it elsewhere)
  Instruction *sumLink(Readers &rd, AddrType sum, uint32_t mod, bool eitherSide, AddrType &other) const {
    Instruction *add = soleReader(rd, sum, EWE_ADD, mod);
    if (!add) return nullptr;
    const bool asA = add->operandList[0] == sum;
    if (!asA && (!eitherSide || add->operandList[2] != sum)) return nullptr;
    other = asA ? add->operandList[2] : add->operandList[0];
    return other == sum ? nullptr : add;
  }
  // the MUL_CONST record that produces `a`, if `reader` is all that reads `a`.  ((5a) used to ask !fusedTensor as well: only pass (5) sets that,
  // and only on MAC2 records)
  Instruction *privateScaled(Readers &rd, AddrType a, Instruction *reader, uint32_t mod) const {
    Instruction *m = producerOf(a);
    return m && live(m) && isScaled(m, mod) && onlyReader(rd, a, reader) ? m : nullptr;
  }
  // the ADD_CONST record that is the only reader of `sum`
  Instruction *constTail(Readers &rd, AddrType sum, uint32_t mod) const {
    Instruction *k = soleReader(rd, sum, EWE_ADD_CONST, mod);
    return k && k->hasConstant ? k : nullptr;
  }
  // the record `c` that absorbs others: it ends up where the last of them stood, with the outputs it is given
  struct Absorber {
    Planner &P;
    Readers &rd;
    Placement &place;
    Instruction *c, *last;
    Absorber(Planner &p, Readers &r, Placement &pl, Instruction *carrier) : P(p), rd(r), place(pl), c(carrier), last(carrier) {}
    void take(Instruction *i) {
      P.absorb(c, i);
      if (place.after(i, last)) last = i;
    }
    // the same scalar behind the three polynomials d: their MUL_CONST records go in, d moves behind them
    bool takeScalars(Triple &d, uint64_t &s) {
      Three m;
      if (!P.scalars(rd, d, c->mod_id, m)) return false;
      s = m[0]->constant;
      for (int i = 0; i < 3; ++i) { take(m[i]); d[i] = m[i]->OutputOperand; }
      return true;
    }
    // ((5m), (5a)) addend after addend, up to `max`: d0 and d1 each go on through ONE ADD whose other operand is a MUL_CONST record read by nothing
    // else, both with the same constant u (u x onto d0, u y onto d1).  An addend goes in with both its components or not at all
    void takeAddends(AddrType &d0, AddrType &d1, uint32_t max) {
      Fused &f = c->fu;
      while (f.addends < max) {
        AddrType x0 = 0, x1 = 0;
        Instruction *a0 = P.sumLink(rd, d0, c->mod_id, true, x0), *a1 = P.sumLink(rd, d1, c->mod_id, true, x1);
        Instruction *u0 = a0 ? P.privateScaled(rd, x0, a0, c->mod_id) : nullptr, *u1 = a1 ? P.privateScaled(rd, x1, a1, c->mod_id) : nullptr;
        if (!u0 || !u1 || u0->constant != u1->constant) break;
        f.reads.push_back(u0->operandList[0]);
        f.reads.push_back(u1->operandList[0]);
        f.scales2.push_back(u0->constant);
        ++f.addends;
        for (Instruction *i : {u0, a0, u1, a1}) take(i);
        d0 = a0->OutputOperand; d1 = a1->OutputOperand;
      }
    }
    // the ADD_CONST behind `sum` goes in, `sum` moves behind it
    void takeConstant(AddrType &sum) {
      if (Instruction *k = P.constTail(rd, sum, c->mod_id)) {
        c->fu.hasConst = true;
        c->fu.constant = k->constant;
        take(k);
        sum = k->OutputOperand;
      }
    }
    // the outputs of the finished record; it is the producer of every one of them.  (The passes with one output, (5l) and (5c), used to re-point
    // `producer` for that one only: their records have no other write, so this is the same)
    void finish(AddrType out, const std::vector<AddrType> &extra) {
      c->OutputOperand = out;
      c->extraOutputs = extra;
      for (const Write &w : recordWrites(*c)) P.producer[w.addr] = c;
      place.moveTo(c, last);   // to where its last link stood
    }
    void finish(const Triple &d) { finish(d[1], {d[0], d[2]}); }
  };

  void passThrough();      // 1
  void inttScale();        // 2
  void eweChains();        // 3
  void nttSubScale();      // 4
  void productOperands();  // 4p
  void mergeRescale();     // 4b
  void residue();          // 4c
  void tensor();           // 5
  void tensorDot();        // 5d
  void tensorSquare();     // 5q
  void linearCombination();   // 5l
  void multiCombination();    // 5L
  void tensorMulAdd();     // 5m
  void realImaginary();    // 5r
  void complexCombination();   // 5c
  void plaintextCombination(); // 5p
  void tensorDotAdd();     // 5a
  void keyProduct();       // 6
  // what (6m/6l), (6s) and (6h) all recognise: the live two-key key-product records whose digits are all automorphisms, by one element per record, of
  // the same materialised digits and are read by nothing else; per (modulus, unrotated digits) the records and their automorphisms, in stage order
  typedef std::pair<uint32_t, std::vector<AddrType>> DigitsKey;
  typedef std::vector<std::pair<Instruction *, std::vector<Instruction *>>> Rotations;
  struct RotationGroups {
    std::map<DigitsKey, Rotations> members;
    std::vector<DigitsKey> order;   // first appearance
  };
  RotationGroups rotationGroups(Readers &rd);
  // two records by one element are not rotations of one ciphertext
  static bool distinctElements(const Rotations &mem, size_t b, size_t e) {
    std::set<uint32_t> distinct;
    for (size_t m = b; m < e; ++m) distinct.insert(mem[m].second[0]->galois);
    return distinct.size() == e - b;
  }
  void weightedRotations(size_t minSums, size_t maxSums);   // 6m (several sums) and 6l (one)
  void sumOfRotations();      // 6s
  void hoist();               // 6h
  void transformTimesKey();   // 7 + 8
  void keyProductInverseOut();   // 7b
  void modDownConversion();   // 9
  void conversionEpilogue();  // 10
  void packConversionInputs();   // 11
  void foldAutomorphisms();   // 12
  void sweep();
};

void Arch::fusePasses(std::vector<Stage> &st) {
  Planner p(*this, st);
  const bool oneGpuKernels = world_ == 1 || shardGather;   // the plans whose conversions run in the one-GPU kernels
  p.passThrough();
  p.inttScale();
  p.eweChains();
  p.nttSubScale();
  if (fusePmulRescale && world_ == 1) p.productOperands();   // behind (4): it reads the fused transforms; in front of (4b): plain records stay (4b)'s
  p.mergeRescale();
  p.residue();
  p.tensor();
  if (fuseDot) p.tensorDot();   // before (6): the multiply-accumulate chains it absorbs are not key products
  if (fuseSquare) p.tensorSquare();
  if (fuseLincomb) p.linearCombination();
  if (fuseMlincomb) p.multiCombination();   // behind (5l): it merges the records (5l) formed
  if (fuseMuladd) p.tensorMulAdd();
  if (fuseReim) p.realImaginary();
  if (fuseClincomb) p.complexCombination();
  if (fusePlincomb) p.plaintextCombination();
  if (fuseDotadd) p.tensorDotAdd();
  p.keyProduct();
  // (6m, 6l) before (6s) and (6h): the records it merges are the ones (6h) would claim, and none of them is (6s)'s (their outputs go into products,
  // not into sums).  fuse_bsgs: the groups with several sums, fuse_lintrans: the ones with one
  if (fuseBsgs || fuseLintrans) p.weightedRotations(fuseLintrans ? 1 : 2, fuseBsgs ? HM_IP_LINTRANS_MULTI_MAX_OUT : 1);
  if (fuseRotsum) p.sumOfRotations();   // before (6h): each record it merges is a group of one rotation to it
  if (fuseHoist) p.hoist();
  if (fuseHpip) p.transformTimesKey();
  if (fuseHpip && fuseIpInv && oneGpuKernels && p.cap("cap_ip_inverse_out")) p.keyProductInverseOut();
  if (fuseBconv && fuseModDown && oneGpuKernels && p.cap("cap_bconv_col_max_in_mix")) p.modDownConversion();
  if (fuseBconv && oneGpuKernels) p.conversionEpilogue();
  if (packBconvIn && oneGpuKernels) p.packConversionInputs();
  if (fuseAuto) p.foldAutomorphisms();
  p.sweep();
}

// (1) pass-through NTT records: consumers read the source directly.
//     Reads: passthrough (generators).  Sets: operandList of every consumer.
void Arch::Planner::passThrough() {
  std::map<AddrType, AddrType> alias;
  for (auto &s : st)
    for (Instruction *i : s.ins)
      if ((i->ops == NTT) && i->passthrough) {
        alias[i->OutputOperand] = i->operandList[0];
        dead.insert(i);
      }
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (dead.count(i)) continue;
      for (AddrType &a : i->operandList) {
        auto al = alias.find(a);
        if (al != alias.end()) a = al->second;
      }
    }
}

// (2) INTT followed by a single MUL_CONST consumer: the constant goes into the INTT epilogue.
//     Sets on the INTT: hasConstant, constant, OutputOperand.
void Arch::Planner::inttScale() {
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (i->ops != MULT || i->opcode != EWE_MUL_CONST || dead.count(i)) continue;
      auto p = producer.find(i->operandList[0]);
      if (p == producer.end() || p->second->ops != INTT || uses[i->operandList[0]] != 1 || p->second->hasConstant) continue;
      p->second->hasConstant = true;
      p->second->constant = i->constant;
      p->second->OutputOperand = i->OutputOperand;
      p->second->refInstructions += i->refInstructions;
      producer[i->OutputOperand] = p->second;
      dead.insert(i);
    }
}

// (3) EWE chains: SUB then MUL_CONST -> SUB_SCALE ; SUB_SCALE then ADD -> SUB_SCALE_ADD.
//     Sets on the surviving MULT record: opcode, operandList, hasConstant, constant.
void Arch::Planner::eweChains() {
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (i->ops != MULT || dead.count(i)) continue;
      if (i->opcode == EWE_MUL_CONST) {
        auto p = producer.find(i->operandList[0]);
        if (p == producer.end() || p->second->ops != MULT || p->second->opcode != EWE_SUB || dead.count(p->second) ||
            uses[i->operandList[0]] != 1)
          continue;
        Instruction *sub = p->second;
        i->opcode = EWE_SUB_SCALE;
        i->operandList[0] = sub->operandList[0];
        i->operandList[2] = sub->operandList[2];
        i->refInstructions += sub->refInstructions;
        dead.insert(sub);
      } else if (i->opcode == EWE_ADD) {
        for (int side = 0; side < 2; ++side) {
          const int me = side ? 2 : 0, other = side ? 0 : 2;
          auto p = producer.find(i->operandList[me]);
          if (p == producer.end() || p->second->ops != MULT || p->second->opcode != EWE_SUB_SCALE || dead.count(p->second) ||
              uses[i->operandList[me]] != 1)
            continue;
          Instruction *ss = p->second;
          const AddrType addend = i->operandList[other];
          i->opcode = EWE_SUB_SCALE_ADD;
          i->operandList[0] = ss->operandList[0];
          i->operandList[2] = ss->operandList[2];
          i->operandList[3] = addend;
          i->hasConstant = true;
          i->constant = ss->constant;
          i->refInstructions += ss->refInstructions;
          dead.insert(ss);
          break;
        }
      }
    }
}

// (4) forward NTT whose only consumer is (minuend - x) * k [+ addend]: the epilogue moves into the transform's
//     last pass (ModDowNTT + ModDownSub + final add; Rescale_NTT + Rescale_SUB + Rescale_Mul).
//     Reads: the SUB_SCALE[_ADD] records of (3).  Sets on the NTT: fusedSubScale, fMinuend, fAddend, hasConstant, constant, OutputOperand.
void Arch::Planner::nttSubScale() {
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (i->ops != MULT || dead.count(i) || (i->opcode != EWE_SUB_SCALE && i->opcode != EWE_SUB_SCALE_ADD)) continue;
      auto p = producer.find(i->operandList[2]);
      if (p == producer.end() || p->second->ops != NTT || p->second->passthrough || dead.count(p->second) ||
          p->second->fusedSubScale || uses[i->operandList[2]] != 1)
        continue;
      Instruction *t = p->second;
      const AddrType minuend = i->operandList[0], addend = i->opcode == EWE_SUB_SCALE_ADD ? i->operandList[3] : 0;
      const AddrType out = i->OutputOperand;
      if (out == t->operandList[0] || out == minuend || out == addend) continue;  // out doubles as first-pass scratch
      t->fusedSubScale = true;
      t->fMinuend = minuend;
      t->fAddend = addend;
      t->hasConstant = true;
      t->constant = i->constant;
      t->OutputOperand = out;
      t->refInstructions += i->refInstructions;
      producer[out] = t;
      dead.insert(i);
    }
}

// (4p) product operands of transforms (pmult with rescale = 1): an EWE_MUL of two operands that nothing in the plan produces (op inputs), read
//      by ONE record, is formed by that reader while it loads:
//        a fused forward transform of (4) without conversion or gathered addend whose minuend it is: out = (a * b - NTT(x)) * k [+ addend];
//        an inverse transform whose input it is: out = INTT(a * b) * N^-1 [* scale].
//      The product limb-poly is never written nor read back.  The tensor MULs of hmult / hdot never match: (5) absorbs them later, and here
//      their outputs are minuends of nothing ((4)'s minuend is the key-switch sum) or have a second reader.
//      Reads: fusedSubScale / fMinuend (4).  Sets: fMinuendB + fMinuend on forward transforms, inMulB + operandList[0] on inverse transforms.
void Arch::Planner::productOperands() {
  Readers rd = readers();
  if (A.fusePmulAuto && A.genericArith) {
    // Not told either way, on the generic back-end: its one-launch transform has no product form (the extra operand costs that kernel a wave per
    // SIMD), so a final launch inside the one-launch limit would trade the one-launch MODE 3 transform for two 16-coefficient kernels: measured
    // equal to the three-launch plan.  The pass keeps out; larger launches are 16-coefficient kernels either way
    size_t finals = 0;
    for (auto &s : st)
      for (Instruction *i : s.ins) finals += live(i) && i->ops == NTT && i->fusedSubScale && !i->passthrough;
    if (finals * A.batch_ <= cap("cap_ntt_fused_small")) return;
  }
  auto productFor = [&](AddrType a, Instruction *reader) -> Instruction * {
    Instruction *m = producerOf(a);
    if (!m || !isMul(m, reader->mod_id) || m->fusedTensor || m->mark == FusedForm::PLincomb || !onlyReader(rd, a, reader)) return nullptr;   // (a one-term hplincomb keeps its own launch: (5p))
    if (producerOf(m->operandList[0]) || producerOf(m->operandList[1])) return nullptr;
    return m;
  };
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (!live(i) || i->passthrough) continue;
      if (i->ops == NTT && i->fusedSubScale && !i->fMinuendB && i->fConvIn.empty() && !i->fAddendGalois) {
        Instruction *m = productFor(i->fMinuend, i);
        if (!m || m->operandList[0] == i->OutputOperand || m->operandList[1] == i->OutputOperand) continue;   // out doubles as first-pass scratch
        i->fMinuend = m->operandList[0];
        i->fMinuendB = m->operandList[1];
        absorb(i, m);
      } else if (i->ops == INTT && !i->secondOnly && !i->inGalois && !i->inMulB) {
        Instruction *m = productFor(i->operandList[0], i);
        if (!m) continue;
        i->operandList[0] = m->operandList[0];
        i->inMulB = m->operandList[1];
        absorb(i, m);
      }
    }
}

// (4b) ModDown finish followed by the rescale of the same limb.  T: h = (ip - NTT(conv)) * kT + d and
//      R: out = (h - NTT(r)) * kR with r = INTT(last limb of h) are both linear in the coefficient domain:
//      out = (ip - NTT(conv + kT^-1 * r)) * (kT kR) + d * kR — ONE transform per limb instead of two, and h never
//      exists (the last limb keeps T: r comes from it).  Bit-identical: everything is exact modular arithmetic.
//      Reads: the fused transforms of (4).  Sets on R: fMix, fMixConst, fAddendConst, operandList[0], fMinuend, fAddend, constant.
void Arch::Planner::mergeRescale() {
  for (auto &s : st)
    for (Instruction *R : s.ins) {
      if (R->ops != NTT || !R->fusedSubScale || R->fAddend || R->fMix || dead.count(R)) continue;
      auto p = producer.find(R->fMinuend);
      if (p == producer.end() || p->second == R || !p->second->fusedSubScale || p->second->fMix || dead.count(p->second) ||
          p->second->mod_id != R->mod_id || uses[R->fMinuend] != 1)
        continue;
      Instruction *T = p->second;
      const uint64_t q = A.modulus(R->mod_id);
      // R survives (its stage comes after the INTT that produces r, so the stage list stays a topological order)
      R->fMix = R->operandList[0];
      R->fMixConst = hm::invmod(T->constant, q);
      R->operandList[0] = T->operandList[0];
      R->fMinuend = T->fMinuend;
      R->fAddend = T->fAddend;
      R->fAddendConst = T->fAddend ? R->constant : 0;
      R->constant = hm::mulmod(T->constant, R->constant, q);
      R->refInstructions += T->refInstructions;
      dead.insert(T);
    }
}

// (4c) the residue r = INTT(h_last) that the merged records mix in.  h_last = (ip - NTT(conv)) * kT + d is only ever
//      needed in coefficient form, where it is (INTT(ip) - conv) * kT + INTT(d): conv never has to be transformed and
//      brought back.  INTT(ip) and INTT(d) depend on nothing after the inner product, so they join the ModDown INTT
//      launch (equal dependency depth), and one element-wise SUB_SCALE_ADD on the last limb replaces the two
//      latency-bound single-limb transforms T_last and INTT(h_last).
//      Reads: fMix of (4b), the fused transform of (4).  Adds records (two INTT, one MULT) to the stage of the INTT it replaces and
//      a limb of its own for INTT(d_last).
void Arch::Planner::residue() {
  struct Rewrite { Instruction *T, *X; size_t stage; };
  std::vector<Rewrite> todo;
  for (size_t si = 0; si < st.size(); ++si)
    for (Instruction *X : st[si].ins) {
      if (X->ops != INTT || X->hasConstant || dead.count(X)) continue;
      auto p = producer.find(X->operandList[0]);
      if (p == producer.end() || dead.count(p->second) || !p->second->fusedSubScale || p->second->fMix || p->second->ops != NTT ||
          uses[X->operandList[0]] != 1)
        continue;
      bool mixedIn = false;
      for (auto &s2 : st)
        for (Instruction *i : s2.ins) mixedIn |= !dead.count(i) && i->fMix == X->OutputOperand;
      if (mixedIn) todo.push_back(Rewrite{p->second, X, si});
    }
  AddrType fresh = A.limbIndex.empty() ? 1 : A.limbIndex.rbegin()->first + 1;
  for (const Rewrite &w : todo) {
    Instruction *T = w.T, *X = w.X;
    const AddrType h = X->operandList[0], r = X->OutputOperand;
    Instruction *ia = new Instruction("INTT", INTT, T->level_id);   // wa = INTT(ip_last), kept in h's limb
    ia->mod_id = T->mod_id; ia->operandList = {T->fMinuend}; ia->OutputOperand = h; ia->refInstructions = T->refInstructions;
    st[w.stage].ins.push_back(ia);
    AddrType wb = 0;
    if (T->fAddend) {                                               // wb = INTT(d_last), in a limb of its own
      wb = fresh++;
      A.registerLimbs({wb});
      Instruction *ib = new Instruction("INTT", INTT, T->level_id);
      ib->mod_id = T->mod_id; ib->operandList = {T->fAddend}; ib->OutputOperand = wb;
      st[w.stage].ins.push_back(ib);
    }
    Instruction *e = new Instruction("MULT", MULT, T->level_id);    // r = (wa - conv_last) * kT [+ wb]
    e->mod_id = T->mod_id;
    e->opcode = wb ? EWE_SUB_SCALE_ADD : EWE_SUB_SCALE;
    e->operandList = {h, 0, T->operandList[0], wb};
    e->hasConstant = true; e->constant = T->constant;
    e->OutputOperand = r; e->refInstructions = X->refInstructions;
    st[w.stage].ins.push_back(e);
    producer[h] = ia; producer[r] = e;
    dead.insert(T); dead.insert(X);
  }
}

// (5) tensor product: d1 = p*s + r*t (MAC2) with d0 = p*t and d2 = r*s (MUL) of the same limb -> one pass.
//     Sets on the MAC2 record: fusedTensor, extraOutputs.
void Arch::Planner::tensor() {
  // (several MULs of the same two operands: the pairs of an hdotadd whose inputs are bound to the same ciphertexts; each MAC2 takes one of its own)
  std::map<std::pair<AddrType, AddrType>, std::vector<Instruction *>> muls;
  for (auto &s : st)
    for (Instruction *i : s.ins)
      if (i->ops == MULT && i->opcode == EWE_MUL && !dead.count(i)) muls[{i->operandList[0], i->operandList[1]}].push_back(i);
  auto mulOf = [&](AddrType x, AddrType y, uint32_t mod, Instruction *besides) -> Instruction * {
    auto m = muls.find({x, y});
    if (m == muls.end()) return nullptr;
    for (Instruction *i : m->second)
      if (i != besides && !dead.count(i) && i->mod_id == mod) return i;
    return nullptr;
  };
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (i->ops != MULT || i->opcode != EWE_MAC2 || dead.count(i)) continue;
      const AddrType P = i->operandList[0], S = i->operandList[1], R = i->operandList[2], T = i->operandList[3];
      Instruction *u = mulOf(P, T, i->mod_id, nullptr), *v = mulOf(R, S, i->mod_id, u);
      if (!u || !v) continue;
      i->fusedTensor = true;
      i->extraOutputs = {u->OutputOperand, v->OutputOperand};
      i->refInstructions += u->refInstructions + v->refInstructions;
      dead.insert(u);
      dead.insert(v);
    }
}

// (5d) sum of tensor products (hdot): behind a tensor record of (5) whose MAC2 is marked as pair 1 of a sum (mark TensorDot), pair after pair, d0 and d2
//      go on through ONE MAC_ADD each (d0 += c00 c10, d2 += c01 c11) and d1 through ONE ADD of a MAC2 of the same four operands
//      (c00 c11 + c01 c10); every intermediate is read only by the next link.  The links that agree on their four operands, pair by pair, merge
//      WITH the tensor record into one record per limb: hm_tensor_dot sums the raw products of all pairs and stores the three final sums only.
//      Never written: the three outputs of every pair but the last, and the per-pair MAC2.  The record takes the place of the last record it
//      absorbs in the stage list: every operand of every pair is older, every reader of the sums comes after the chains' ends.
//      Reads: fusedTensor / extraOutputs (5).  Sets on the tensor record: fu (form TensorDot: reads, terms), OutputOperand, extraOutputs.
void Arch::Planner::tensorDot() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::TensorDot)) {
    if (!c->fusedTensor) continue;
    Absorber ab(*this, rd, place, c);
    Fused &f = c->fu;
    f.form = FusedForm::TensorDot;
    f.reads = pairOperands(c);   // pair 1
    f.terms = 1;
    Triple d = tensorOutputs(c);
    while (f.terms < HM_TENSOR_DOT_MAX_TERMS) {
      Instruction *m0 = soleReader(rd, d[0], EWE_MAC_ADD, c->mod_id), *m2 = soleReader(rd, d[2], EWE_MAC_ADD, c->mod_id);
      AddrType other = 0;
      Instruction *add = sumLink(rd, d[1], c->mod_id, true, other);
      if (!m0 || !m2 || !add || m0->operandList[2] != d[0] || m2->operandList[2] != d[2]) break;
      Instruction *mac = producerOf(other);
      if (!mac || !live(mac) || mac->ops != MULT || mac->opcode != EWE_MAC2 || mac->fusedTensor || mac->mod_id != c->mod_id || !onlyReader(rd, other, add)) break;
      const AddrType c00 = m0->operandList[0], c10 = m0->operandList[1], c01 = m2->operandList[0], c11 = m2->operandList[1];
      if (mac->operandList[0] != c00 || mac->operandList[1] != c11 || mac->operandList[2] != c01 || mac->operandList[3] != c10) break;
      f.reads.insert(f.reads.end(), {c00, c10, c01, c11});
      ++f.terms;
      for (Instruction *i : {m0, m2, mac, add}) ab.take(i);
      d = {m0->OutputOperand, add->OutputOperand, m2->OutputOperand};
    }
    ab.finish(d);
  }
}

// (5q) scaled square plus constant (hsquare): a tensor record of (5) that the builder marked (mark Square) and whose operand pairs coincide
//      (c00 == c10, c01 == c11: a ciphertext times itself) becomes a record of hm_tensor_square, which reads each polynomial once.  Behind it,
//      the MUL_CONST records that are the only readers of its three outputs go in when all three carry the same constant (s d0, s d1, s d2), then the
//      ADD_CONST record that is the only reader of d0 (d0 + k).  The record's outputs become the final buffers, so every later pass sees what it
//      sees in hmult; it takes the place of the last record it absorbs.  Never written: the products in front of the scalar and of the constant.
//      Reads: fusedTensor / extraOutputs (5).  Sets on the tensor record: fu (form Square: reads, hasScale, scales, hasConst, constant), OutputOperand,
//      extraOutputs.
void Arch::Planner::tensorSquare() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::Square)) {
    const std::vector<AddrType> pair = pairOperands(c);
    if (!c->fusedTensor || pair[0] != pair[1] || pair[2] != pair[3]) continue;
    Absorber ab(*this, rd, place, c);
    Fused &f = c->fu;
    f.form = FusedForm::Square;
    f.reads = {pair[0], pair[2]};
    f.scales = {1};
    Triple d = tensorOutputs(c);
    f.hasScale = ab.takeScalars(d, f.scales[0]);
    ab.takeConstant(d[0]);
    ab.finish(d);
  }
}

// (5l) sum of scaled polynomials plus constant (hlincomb): from a MUL_CONST record that the builder marked as term 1 of a sum (mark Lincomb), term
//      after term, the running sum goes on through ONE ADD whose other operand is a MUL_CONST record of the same modulus read by nothing else;
//      behind the last term, ONE ADD_CONST.  Every intermediate is read only by the next link.  The links merge into the marked record:
//      hm_lincomb sums the raw products s_t x_t of all terms, adds the constant and stores the final sum only.  Never written: the T scaled
//      polynomials and the T - 1 partial sums (and the sum in front of the constant).  The record takes the place of the last record it absorbs.
//      Only the builder of HLINCOMB sets the mark: the pass matches nothing in any other op.
//      Sets on the marked record: fu (form Lincomb: reads, scales, terms, hasConst, constant), OutputOperand.
void Arch::Planner::linearCombination() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::Lincomb)) {
    if (!isScaled(c, c->mod_id)) continue;
    Absorber ab(*this, rd, place, c);
    Fused &f = c->fu;
    f.form = FusedForm::Lincomb;
    f.reads = {c->operandList[0]};
    f.scales = {c->constant};
    f.terms = 1;
    AddrType sum = c->OutputOperand;
    while (f.terms < HM_LINCOMB_MAX_TERMS) {
      AddrType other = 0;
      Instruction *add = sumLink(rd, sum, c->mod_id, true, other);
      Instruction *mul = add ? privateScaled(rd, other, add, c->mod_id) : nullptr;
      if (!mul || mul->mark == FusedForm::Lincomb) break;
      f.reads.push_back(mul->operandList[0]);
      f.scales.push_back(mul->constant);
      ++f.terms;
      ab.take(mul);
      ab.take(add);
      sum = add->OutputOperand;
    }
    ab.takeConstant(sum);
    ab.finish(sum, {});
  }
}

// (5L) several sums of scaled polynomials over the same inputs (hmlincomb): the live (5l) records of one modulus whose reads (fu.reads) are the same list
//      in the same order merge, up to HM_LINCOMB_MULTI_MAX_OUT at a time, into the first of them: hm_lincomb_multi loads every input once per
//      tile of outputs and stores every sum once.  The merged record carries the outputs, the scalar rows and the constants in the order the sums
//      stand in the stages, the refInstructions of everything it absorbs, and takes the place of the last record it absorbs: every input is
//      produced in front of the first of them, and nothing reads an output in front of the last (the builder emits every sum before anything that
//      reads one).  Only HMLINCOMB produces several (5l) records over one operand list: the pass matches nothing in any other op.
//      Sets on the first record: fu (form LincombMulti: rowScales, rowConsts, hasConst), OutputOperand (unchanged), extraOutputs.
void Arch::Planner::multiCombination() {
  Readers rd;   // (no link is followed)
  Placement place(st);
  typedef std::pair<uint32_t, std::vector<AddrType>> Key;
  std::map<Key, std::vector<Instruction *>> members;
  std::vector<Key> order;   // first appearance
  for (auto &s : st)
    for (Instruction *i : s.ins)
      if (live(i) && i->fu.form == FusedForm::Lincomb && i->extraOutputs.empty()) {
        const Key k{i->mod_id, i->fu.reads};
        if (!members.count(k)) order.push_back(k);
        members[k].push_back(i);
      }
  for (const Key &k : order) {
    const std::vector<Instruction *> &mem = members[k];
    for (size_t b = 0; b < mem.size(); b += HM_LINCOMB_MULTI_MAX_OUT) {
      const size_t e = std::min(mem.size(), b + (size_t)HM_LINCOMB_MULTI_MAX_OUT);
      if (e - b < 2) continue;   // one sum: (5l)'s record and launch
      Absorber ab(*this, rd, place, mem[b]);
      Fused &f = ab.c->fu;
      std::vector<AddrType> further;
      for (size_t m = b; m < e; ++m) {
        const Fused &g = mem[m]->fu;   // (m == b: the record's own)
        f.rowScales.push_back(g.scales);
        f.rowConsts.push_back(g.hasConst ? g.constant : 0);
        f.hasConst = f.hasConst || g.hasConst;
        if (m > b) further.push_back(mem[m]->OutputOperand);
        ab.take(mem[m]);
      }
      f.form = FusedForm::LincombMulti;
      ab.finish(ab.c->OutputOperand, further);
    }
  }
}

// (5m) scaled tensor product plus scaled addends plus constant (hmuladd): a tensor record of (5) that the builder marked (mark MulAdd) becomes a
//      record of hm_tensor_muladd.  Behind it, the MUL_CONST records that are the only readers of its three outputs go in when all three carry the
//      same constant (s d0, s d1, s d2).  Then, addend after addend, d0 and d1 each go on through ONE ADD whose other operand is a MUL_CONST record
//      of the same modulus read by nothing else, both with the same constant u_t (u_t x_t onto d0, u_t y_t onto d1): an addend goes in with both
//      its components or not at all, so d0 and d1 absorb the same number of ADDs.  Then the ADD_CONST record that is the only reader of d0.  The
//      record's reads become the four product operands plus the 2A addend operands, its outputs the final buffers, so every later pass sees what
//      it sees in hmult; it takes the place of the last record it absorbs.  Never written: the products in front of the scalar, the 2A scaled
//      addends and the partial sums.  Only the builder of HMULADD sets the mark: the pass matches nothing in any other op.
//      Reads: fusedTensor / extraOutputs (5).  Sets on the tensor record: fu (form MulAdd: reads, addends, scales, scales2, hasScale, hasConst, constant),
//      OutputOperand, extraOutputs.
void Arch::Planner::tensorMulAdd() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::MulAdd)) {
    if (!c->fusedTensor) continue;
    Absorber ab(*this, rd, place, c);
    Fused &f = c->fu;
    f.form = FusedForm::MulAdd;
    f.reads = pairOperands(c);
    f.scales = {1};
    Triple d = tensorOutputs(c);
    f.hasScale = ab.takeScalars(d, f.scales[0]);
    ab.takeAddends(d[0], d[1], HM_TENSOR_MULADD_MAX_ADDENDS);
    ab.takeConstant(d[0]);
    ab.finish(d);
  }
}

// (5a) scaled sum of tensor products plus scaled addends plus constant (hdotadd): a tensor record of (5) that the builder marked (mark DotAdd) becomes
//      a record of hm_tensor_dotadd.  It absorbs, in this order:
//        its three sole-reader MUL_CONST records when all three carry the same constant (s_1 d0, s_1 d1, s_1 d2);
//        pair after pair, the three ADD records that are the only readers of the running d0, d1, d2 and whose other operands are the three
//        outputs of ONE unmarked tensor record of (5) of the same modulus, read by nothing else, either directly or, all three, through a
//        MUL_CONST record of one constant s_t read by nothing else: the tensor record, its MUL_CONSTs and the ADDs go in, all three or none;
//        the addends and the constant, as pass (5m) takes them: per addend ONE ADD on d0 and ONE on d1 whose other operands are MUL_CONST records
//        of the same constant u_r read by nothing else, then the ADD_CONST record that is the only reader of d0.
//      The record's reads become the 4T operands plus the 2A addend operands (recordReads), its outputs the final buffers, so every later pass
//      sees what it sees in hmult; it takes the place of the last record it absorbs and keeps fusedTensor, so pass (6) stays off it.  Never
//      written: the 3T products, their scaled copies, the 2A scaled addends and the partial sums.  Only the builder of HDOTADD sets the mark: the
//      pass matches nothing in any other op.
//      Reads: fusedTensor / extraOutputs (5).  Sets on the marked record: fu (form DotAdd: reads, terms, addends, scales, scales2, hasScale, hasConst, constant),
//      OutputOperand, extraOutputs.
void Arch::Planner::tensorDotAdd() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::DotAdd)) {
    if (!c->fusedTensor) continue;
    Absorber ab(*this, rd, place, c);
    Fused &f = c->fu;
    f.form = FusedForm::DotAdd;
    f.reads = pairOperands(c);
    f.scales = {1};
    f.terms = 1;
    Triple d = tensorOutputs(c);
    f.hasScale = ab.takeScalars(d, f.scales[0]);
    while (f.terms < HM_TENSOR_DOTADD_MAX_TERMS) {
      Three add, mul;
      Triple src;
      bool ok = true;
      for (int i = 0; i < 3 && ok; ++i) ok = (add[i] = sumLink(rd, d[i], c->mod_id, true, src[i])) != nullptr;
      if (!ok) break;
      // through the pair's MUL_CONST records, all three or none
      int scaledOps = 0;
      for (int i = 0; i < 3; ++i)
        if ((mul[i] = privateScaled(rd, src[i], add[i], c->mod_id))) ++scaledOps;
      if (scaledOps != 0 && scaledOps != 3) break;
      Triple prod = src;
      if (scaledOps == 3) {
        if (mul[0]->constant != mul[1]->constant || mul[0]->constant != mul[2]->constant) break;
        for (int i = 0; i < 3; ++i) prod[i] = mul[i]->operandList[0];
      }
      // the three products are the outputs of one unmarked tensor record that no pass has taken, each read by its link only
      Instruction *x = producerOf(prod[1]);
      if (!x || x == c || !live(x) || !x->fusedTensor || x->mark == FusedForm::DotAdd || x->mod_id != c->mod_id || x->fu.form != FusedForm::None ||
          x->extraOutputs.size() != 2 || tensorOutputs(x) != prod)
        break;
      for (int i = 0; i < 3 && ok; ++i) ok = onlyReader(rd, prod[i], scaledOps ? mul[i] : add[i]);
      if (!ok) break;
      const std::vector<AddrType> pair = pairOperands(x);
      f.reads.insert(f.reads.end(), pair.begin(), pair.end());
      f.scales.push_back(scaledOps ? mul[0]->constant : 1);
      ++f.terms;
      if (scaledOps) f.hasScale = true;
      ab.take(x);
      for (int i = 0; i < 3; ++i) {
        if (mul[i]) ab.take(mul[i]);
        ab.take(add[i]);
        d[i] = add[i]->OutputOperand;
      }
    }
    ab.takeAddends(d[0], d[1], HM_TENSOR_DOTADD_MAX_ADDENDS);   // the addends and the constant: (5m)'s
    ab.takeConstant(d[0]);
    ab.finish(d);
  }
}

// (5r) real and imaginary parts (hreim): from an ADD record x + y that the builder marked (mark ReIm), with x an op input's limb and y the limb of
//      its conjugate: the ONE live SUB record x - y of the same two operands, in this order, and modulus, whose output is read by ONE MUL record
//      only, the difference its operand a and its operand b a limb that nothing produces (the stored evaluation form of -X^(N/2)).  The three
//      merge into the marked record: hm_reim_split reads x and y once and stores the sum and the product; the factor is derived by the back-end
//      from its roots, so the fused record does not read the stored one.  Never written: the difference.  The record takes the place of the last
//      record it absorbs.  Only the builder of HREIM sets the mark: the pass matches nothing in any other op.
//      Sets on the marked record: fu (form ReIm: reads), extraOutputs.
void Arch::Planner::realImaginary() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::ReIm)) {
    if (c->ops != MULT || c->opcode != EWE_ADD || !c->extraOutputs.empty()) continue;
    const AddrType x = c->operandList[0], y = c->operandList[2];
    Instruction *sub = nullptr;
    size_t subs = 0;
    for (Instruction *r : rd[x])
      if (r != c && live(r) && r->ops == MULT && r->opcode == EWE_SUB && r->mod_id == c->mod_id && r->operandList[0] == x && r->operandList[2] == y) { sub = r; ++subs; }
    if (subs != 1) continue;
    Instruction *mul = soleReader(rd, sub->OutputOperand, EWE_MUL, c->mod_id);
    if (!mul || mul->operandList[0] != sub->OutputOperand || mul->operandList[1] == sub->OutputOperand || producerOf(mul->operandList[1])) continue;
    Absorber ab(*this, rd, place, c);
    c->fu.form = FusedForm::ReIm;
    c->fu.reads = {x, y};
    ab.take(sub);
    ab.take(mul);
    ab.finish(c->OutputOperand, {mul->OutputOperand});   // (the sum stays the record's own output)
  }
}

// (5c) sum of polynomials times a + b X^(N/2) plus constant (hclincomb): from a MUL_CONST record a_1 x_1 that the builder marked as term 1 of such a
//      sum (mark CLincomb).  A term is the ADD of two MUL_CONST records of the same modulus, each read by nothing else: the real part a_t x_t, and
//      the monomial part whose operand is the output, read by nothing else, of a MUL record of the SAME x_t by a limb that nothing produces (the
//      stored evaluation form of -X^(N/2)); its constant is q - b_t.  Term 1 is the ADD that reads the marked record; term after term, the running
//      sum goes on through ONE ADD whose other operand is such a term, read by nothing else; behind the last term, ONE ADD_CONST.  The links merge
//      into the marked record: hm_clincomb sums the raw products of all terms by the scalar of each half, adds the constant and stores the final
//      sum only; the factor is derived by the back-end from its roots, so the fused record does not read the stored one.  Never written: the 4T
//      parts and the T - 1 partial sums (and the sum in front of the constant).  The record takes the place of the last record it absorbs.
//      Only the builder of HCLINCOMB sets the mark: the pass matches nothing in any other op.
//      Sets on the marked record: fu (form CLincomb: reads, scales, scales2, terms, hasConst, constant), OutputOperand.
void Arch::Planner::complexCombination() {
  Readers rd = readers();
  Placement place(st);
  for (Instruction *c : markedHeads(FusedForm::CLincomb)) {
    if (!isScaled(c, c->mod_id)) continue;
    const uint64_t q = A.modulus(c->mod_id);
    // the records of one term behind its ADD `term`: re, rot, im, or none
    struct Term { Instruction *re = nullptr, *rot = nullptr, *im = nullptr; };
    auto termOf = [&](Instruction *term, Term &t) {
      if (term->operandList[0] == term->operandList[2]) return false;
      t.re = privateScaled(rd, term->operandList[0], term, c->mod_id);
      t.im = privateScaled(rd, term->operandList[2], term, c->mod_id);
      if (!t.re || !t.im || t.im->mark == FusedForm::CLincomb || (t.re->mark == FusedForm::CLincomb && t.re != c)) return false;
      t.rot = producerOf(t.im->operandList[0]);
      return t.rot && isMul(t.rot, c->mod_id) && !t.rot->fusedTensor && onlyReader(rd, t.rot->OutputOperand, t.im) &&
             t.rot->operandList[0] == t.re->operandList[0] && t.rot->operandList[1] != t.rot->operandList[0] && !producerOf(t.rot->operandList[1]);
    };
    Instruction *first = soleReader(rd, c->OutputOperand, EWE_ADD, c->mod_id);
    Term t1;
    if (!first || first->operandList[0] != c->OutputOperand || !termOf(first, t1) || t1.re != c) continue;
    Absorber ab(*this, rd, place, c);
    Fused &f = c->fu;
    f.form = FusedForm::CLincomb;
    auto add = [&](const Term &t) {
      f.reads.push_back(t.re->operandList[0]);
      f.scales.push_back(t.re->constant);
      f.scales2.push_back(t.im->constant ? q - t.im->constant : 0);
      ++f.terms;
      ab.take(t.re); ab.take(t.rot); ab.take(t.im);
    };
    add(t1);   // (re == c: absorbing itself does nothing)
    ab.take(first);
    AddrType sum = first->OutputOperand;
    while (f.terms < HM_CLINCOMB_MAX_TERMS) {
      AddrType other = 0;
      Instruction *link = sumLink(rd, sum, c->mod_id, false, other);
      Instruction *term = link ? producerOf(other) : nullptr;
      Term t;
      if (!term || !live(term) || term->ops != MULT || term->opcode != EWE_ADD || term->mod_id != c->mod_id || term->fusedTensor || !onlyReader(rd, other, link) ||
          !termOf(term, t))
        break;
      add(t);
      ab.take(term);
      ab.take(link);
      sum = link->OutputOperand;
    }
    ab.takeConstant(sum);
    ab.finish(sum, {});
  }
}

// (5p) sum of ciphertexts times plaintexts plus a plaintext on c0 (hplincomb): from a MUL record p_1 (.) x_1 that the builder marked as term 1 of
//      one component's sum (mark PLincomb).  A chain is that record followed, term after term, by ONE MAC_ADD record of the same modulus whose
//      operand c is the running sum, read by nothing else; behind the last term, ONE marked ADD of the sum (operand a) and a limb that nothing
//      produces (the plaintext addend).  Two chains of one modulus whose plaintext limbs (operand b) coincide term by term are the two components
//      of one output limb: they merge into the marked record of the chain that carries the addend, or of the earlier one if neither does.
//      hm_plincomb loads every plaintext pair once for both products, sums the raw products of each component in its own accumulator, adds the
//      addend to c0's and stores the two final sums only.  A chain without a partner stays as it is.  Never written: the 2 (T - 1) partial sums
//      and the sum in front of the addend.  The record takes the place of the last record it absorbs.
//      Only the builder of HPLINCOMB sets the mark: the pass matches nothing in any other op.
//      Sets on the marked record: fu (form PLincomb: reads, terms, hasAddend), OutputOperand, extraOutputs.
void Arch::Planner::plaintextCombination() {
  Readers rd = readers();
  Placement place(st);
  struct Sum { std::vector<Instruction *> terms; Instruction *add = nullptr; };
  typedef std::pair<uint32_t, std::vector<AddrType>> Key;   // modulus, the plaintext limb of every term
  std::map<Key, std::vector<Sum>> byPlain;
  std::vector<Key> order;   // first appearance
  for (Instruction *i : markedHeads(FusedForm::PLincomb)) {
    if (!isMul(i, i->mod_id) || i->fusedTensor) continue;   // (the marked ADD of the addend is no head)
    Sum c;
    c.terms = {i};
    while (c.terms.size() < HM_PLINCOMB_MAX_TERMS) {
      Instruction *next = soleReader(rd, c.terms.back()->OutputOperand, EWE_MAC_ADD, i->mod_id);
      if (!next || next->operandList[2] != c.terms.back()->OutputOperand || next->operandList[0] == next->operandList[2] ||
          next->operandList[1] == next->operandList[2])
        break;
      c.terms.push_back(next);
    }
    AddrType addend = 0;
    Instruction *add = sumLink(rd, c.terms.back()->OutputOperand, i->mod_id, false, addend);
    if (add && add->mark == FusedForm::PLincomb && !producerOf(addend)) c.add = add;
    Key key{i->mod_id, {}};
    for (Instruction *t : c.terms) key.second.push_back(t->operandList[1]);
    if (!byPlain.count(key)) order.push_back(key);
    byPlain[key].push_back(c);
  }
  for (const Key &key : order) {
    std::vector<Sum> &sums = byPlain[key];
    if (sums.size() != 2 || (sums[0].add && sums[1].add)) continue;
    const Sum &s0 = sums[1].add ? sums[1] : sums[0], &s1 = sums[1].add ? sums[0] : sums[1];
    Absorber ab(*this, rd, place, s0.terms[0]);
    Fused &f = ab.c->fu;
    f.form = FusedForm::PLincomb;
    f.terms = (uint32_t)s0.terms.size();
    for (size_t t = 0; t < s0.terms.size(); ++t) f.reads.insert(f.reads.end(), {s0.terms[t]->operandList[1], s0.terms[t]->operandList[0], s1.terms[t]->operandList[0]});
    for (Instruction *i : s0.terms) ab.take(i);
    for (Instruction *i : s1.terms) ab.take(i);
    AddrType out0 = s0.terms.back()->OutputOperand;
    if (s0.add) {
      f.hasAddend = true;
      f.reads.push_back(s0.add->operandList[2]);
      ab.take(s0.add);
      out0 = s0.add->OutputOperand;
    }
    ab.finish(out0, {s1.terms.back()->OutputOperand});
  }
}

// (6) inner product with the evaluation key: the chain MAC2 / MAC_ADD ... of one key collapses into a single sum
//     of products, and the two keys (same ext operands) into one two-output record (the HPIP unit's job).
//     Two chains whose second operands are all weights shared between sums (unproduced, with further MUL / MAC_ADD readers) are left alone: the
//     weighted sums of hbsgs share their terms between groups and their plaintexts between sums; a key limb has one reader.
//     Reads: fusedTensor (5).  Sets on the later chain's last record: ops = IP, ipX, ipY, OutputOperand, extraOutputs.
void Arch::Planner::keyProduct() {
  struct Dot { std::vector<AddrType> x, y; std::vector<Instruction *> members; };
  std::map<Instruction *, Dot> dots;
  auto single = [&](AddrType a) { return uses[a] == 1; };
  std::vector<Instruction *> order;
  for (auto &s : st)
    for (Instruction *i : s.ins) order.push_back(i);
  for (Instruction *i : order) {
    if (i->ops != MULT || dead.count(i) || i->fusedTensor) continue;
    Dot d;
    if (i->opcode == EWE_MUL) { d.x = {i->operandList[0]}; d.y = {i->operandList[1]}; }
    else if (i->opcode == EWE_MAC2) { d.x = {i->operandList[0], i->operandList[2]}; d.y = {i->operandList[1], i->operandList[3]}; }
    else if (i->opcode == EWE_MAC_ADD) {
      auto p = producer.find(i->operandList[2]);
      if (p == producer.end() || !dots.count(p->second) || !single(i->operandList[2]) || p->second->mod_id != i->mod_id) continue;
      d = dots[p->second];
      d.x.push_back(i->operandList[0]);
      d.y.push_back(i->operandList[1]);
    } else continue;
    d.members.push_back(i);
    dots[i] = d;
  }
  // keep the dots that end a chain (nobody extends them) and have a partner with the same x list or >= 3 terms
  Readers rd = readers();   // as the records stand in front of this pass
  std::set<Instruction *> extended;
  for (auto &kv : dots)   // (fills a set: the iteration order leaks nowhere)
    for (size_t m = 0; m + 1 < kv.second.members.size(); ++m) extended.insert(kv.second.members[m]);
  std::map<std::pair<uint32_t, std::vector<AddrType>>, Instruction *> byX;
  for (Instruction *i : order) {
    auto it = dots.find(i);
    if (it == dots.end() || extended.count(i) || it->second.x.size() > 4) continue;
    Dot &d = it->second;
    auto key = std::make_pair(i->mod_id, d.x);
    auto partner = byX.find(key);
    if (partner == byX.end()) { byX[key] = i; continue; }
    Instruction *a = partner->second;  // first key
    Dot &da = dots[a];
    if (a->ops == IP) continue;        // already paired
    // Two chains that share their terms are NOT the two keys of a key product when every second operand of the later one is a weight shared
    // between sums: nobody produces it and it has further readers, all of them MUL / MAC_ADD records that multiply by it too (hbsgs: the
    // plaintext limbs of group m, read by its S_0, S_1 and U chains).  Those chains are (6m)'s.  The rule holds for every op and whatever
    // fuse_bsgs says (the chains then stay element-wise); a key limb has one reader, so no key product of an existing op meets it, and an op
    // that one day shares key limbs between two key products in exactly this way would have to be told apart here
    auto sharedWeight = [&](AddrType y) {
      auto &r = rd[y];
      return r.size() > 1 && !producerOf(y) && std::all_of(r.begin(), r.end(), [&](Instruction *u) {
        return u->ops == MULT && (u->opcode == EWE_MUL || u->opcode == EWE_MAC_ADD) && u->operandList[1] == y; });
    };
    if (std::all_of(d.y.begin(), d.y.end(), sharedWeight)) continue;
    // `i` (the later one) carries the fused record so that it is scheduled after every member of both chains
    const AddrType outFirst = a->OutputOperand, outSecond = i->OutputOperand;
    i->ops = IP;
    i->ipX = d.x;
    i->ipY = {da.y, d.y};
    i->OutputOperand = outFirst;
    i->extraOutputs = {outSecond};
    producer[outFirst] = i;
    for (Instruction *m : da.members) { i->refInstructions += m->refInstructions; dead.insert(m); }
    for (Instruction *m : d.members)
      if (m != i) { i->refInstructions += m->refInstructions; dead.insert(m); }
    byX.erase(partner);
  }
}

// the rotations of one ciphertext that share their ModUp, as (6l) and (6h) find them (declared with the passes above)
Arch::Planner::RotationGroups Arch::Planner::rotationGroups(Readers &rd) {
  RotationGroups g;
  for (auto &s : st)
    for (Instruction *ip : s.ins) {
      if (!isKeyProduct(*ip) || dead.count(ip) || ip->ipY.size() != 2 || ip->ipXGalois || !ip->ipHoistG.empty() || transformsInside(*ip)) continue;
      std::vector<AddrType> src;
      std::vector<Instruction *> autos;
      for (AddrType x : ip->ipX) {
        Instruction *a = producerOf(x);
        if (!a || a->ops != AUTO || dead.count(a) || a->galois <= 1 || a->mod_id != ip->mod_id || (!autos.empty() && a->galois != autos[0]->galois) ||
            !onlyReader(rd, x, ip))
          break;
        src.push_back(a->operandList[0]);
        autos.push_back(a);
      }
      if (autos.size() != ip->ipX.size()) continue;
      const DigitsKey key(ip->mod_id, src);
      if (!g.members.count(key)) g.order.push_back(key);
      g.members[key].push_back({ip, autos});
    }
  return g;
}

// (6m, 6l) M weighted sums of the SAME rotations, minSums <= M <= maxSums (6m: M >= 2, hbsgs's baby step; 6l: M = 1, hlintrans): the records (6h)
//      would merge, when every rotation's two outputs are read by exactly M chains MUL, MAC_ADD ... against operands nobody produces (plaintexts),
//      S_{m,k} = sum_r acc_{r,k} * pt_{m,r}, chain m using the same plaintext limb for k = 0 and k = 1 at every rotation, merge WITH all 2M chains
//      into one record per (modulus, digit list): hm_inner_product_lintrans (M = 1) / hm_inner_product_lintrans_multi form every rotation's key
//      product once and the M weighted sums in registers, and store the S_{m,k} only.  If every group m also has a chain that multiplies its
//      plaintext limbs with automorphisms, by the rotations' elements, of ONE source (the Q limbs: U_m = sum_r sigma_r(c0) * pt_{m,r}; the M chains
//      share the R automorphisms), the M chains join as addend outputs: all of them or none.  Never written: the rotated digits, the per-rotation
//      sums, the rotated c0.  The first key-product record in stage order carries the merged one: everything it reads is older, every reader of
//      S_{m,k} and U_m comes after the chains' ends.
//      The identity step (identity = 1): a U chain may start one link earlier, with a MUL of the rotations' source itself against a plaintext limb
//      of its own; it then brings the lone MUL W_m of that limb with a second source (the unrotated c1) along, as a fourth output per group.
//      Reads: the key-product records of (6).  Sets on the carrying record: ipX (the unrotated digits), ipY, ipHoistG, ipLinPt ([m][r]), ipLinAddend,
//      ipLinIdPt ([m]), ipLinAddend1, OutputOperand, extraOutputs (group-major).  A non-empty ipHoistG keeps (7), (7b) and (12) off it.
void Arch::Planner::weightedRotations(size_t minSums, size_t maxSums) {
  Readers rd = readers();
  RotationGroups found = rotationGroups(rd);
  for (const DigitsKey &key : found.order) {
    const auto &mem = found.members[key];
    const size_t R = mem.size();
    if (R > HM_IP_LINTRANS_MAX_ROT || !distinctElements(mem, 0, R)) continue;
    auto outOf = [&](size_t r, size_t k) { return k == 0 ? mem[r].first->OutputOperand : mem[r].first->extraOutputs[0]; };
    const size_t M = rd[outOf(0, 0)].size();
    if (M < minSums || M > maxSums) continue;
    // S_{m,k}: the chains in the stage order of their first links at k = 0; the k = 1 chain of group m is the one with group m's plaintexts
    std::vector<std::array<Chain, 2>> S(M);
    std::vector<std::vector<AddrType>> pt(M);
    bool ok = true;
    for (size_t m = 0; m < M && ok; ++m) {
      Instruction *first = rd[outOf(0, 0)][m];
      ok = isMul(first, key.first) && first->operandList[0] == outOf(0, 0);
      if (!ok) break;
      S[m][0] = chainFrom(rd, first, R);
      ok = S[m][0].size() == R;
      for (size_t r = 0; r < R && ok; ++r) {
        Instruction *l = S[m][0][r];
        ok = l->operandList[0] == outOf(r, 0) && !producerOf(l->operandList[1]);
        if (ok) pt[m].push_back(l->operandList[1]);
      }
    }
    auto &first1 = rd[outOf(0, 1)];
    ok = ok && first1.size() == M;
    for (size_t x = 0; x < M && ok; ++x) {
      ok = isMul(first1[x], key.first) && first1[x]->operandList[0] == outOf(0, 1);
      if (!ok) break;
      size_t m = 0;
      while (m < M && !(S[m][1].empty() && pt[m][0] == first1[x]->operandList[1])) ++m;
      ok = m < M;
      if (!ok) break;
      S[m][1] = chainFrom(rd, first1[x], R);
      ok = S[m][1].size() == R;
      for (size_t r = 0; r < R && ok; ++r) ok = S[m][1][r]->operandList[0] == outOf(r, 1) && S[m][1][r]->operandList[1] == pt[m][r];
    }
    // every rotation's outputs are read by these 2M chains and nothing else
    for (size_t r = 0; r < R && ok; ++r)
      for (size_t k = 0; k < 2 && ok; ++k) {
        auto &readers = rd[outOf(r, k)];
        ok = readers.size() == M;
        for (size_t m = 0; m < M && ok; ++m) ok = std::find(readers.begin(), readers.end(), S[m][k][r]) != readers.end();
      }
    if (!ok) continue;
    // U_m: a third MUL reader of group m's first plaintext limb whose chain multiplies pt_{m,r} with sigma_r of the one source; all or none
    std::vector<Chain> U(M);
    std::vector<Instruction *> addendAutos, idHead(M, nullptr), idW(M, nullptr);   // idHead / idW: the identity step's first link of U_m and its W_m
    AddrType addend = 0;
    bool allU = true;
    for (size_t m = 0; m < M && allU; ++m) {
      for (Instruction *u : rd[pt[m][0]]) {
        if (u == S[m][0][0] || u == S[m][1][0] || !isMul(u, key.first) || u->operandList[1] != pt[m][0]) continue;
        Chain c = chainFrom(rd, u, R);
        std::vector<Instruction *> autos;
        for (size_t r = 0; r < c.size(); ++r) {
          Instruction *l = c[r], *a = producerOf(l->operandList[0]);
          if (l->operandList[1] != pt[m][r] || !a || a->ops != AUTO || !live(a) || a->mod_id != key.first || a->galois != mem[r].second[0]->galois ||
              rd[l->operandList[0]].size() != M || (r && a->operandList[0] != autos[0]->operandList[0]) || (m && a != addendAutos[r]))
            break;
          autos.push_back(a);
        }
        if (autos.size() != R) continue;
        U[m] = c;
        if (m == 0) { addendAutos = autos; addend = autos[0]->operandList[0]; }
        break;
      }
      // the identity step: the chain starts one link earlier, with a MUL of the rotations' SOURCE itself against a plaintext limb of its own (nobody
      // produces it), and that limb's one other reader is the lone MUL W_m of a second source (the unrotated c1): U_m and W_m join together
      for (Instruction *u : rd[pt[m][0]]) {
        if (!U[m].empty()) break;
        if (u == S[m][0][0] || u == S[m][1][0] || u->ops != MULT || soleReader(rd, u->operandList[2], EWE_MAC_ADD, key.first) != u || u->operandList[1] != pt[m][0]) continue;
        Instruction *head = producerOf(u->operandList[2]);
        if (!head || !isMul(head, key.first) || head->fusedTensor || producerOf(head->operandList[1])) continue;
        Chain c = chainFrom(rd, head, R + 1);
        std::vector<Instruction *> autos;
        for (size_t r = 1; r < c.size(); ++r) {
          Instruction *l = c[r], *a = producerOf(l->operandList[0]);
          if (l->operandList[1] != pt[m][r - 1] || !a || a->ops != AUTO || !live(a) || a->mod_id != key.first || a->galois != mem[r - 1].second[0]->galois ||
              rd[l->operandList[0]].size() != M || a->operandList[0] != head->operandList[0] || (m && a != addendAutos[r - 1]))
            break;
          autos.push_back(a);
        }
        auto &idReaders = rd[head->operandList[1]];
        Instruction *w = idReaders.size() == 2 ? idReaders[idReaders[0] == head ? 1 : 0] : nullptr;
        // ... whose source nobody in this plan produces (an op input, as the rotations' source: the carrying record stands in front of
        // everything but the ModUp and must not read what is written behind it)
        if (autos.size() != R || !w || w == head || !isMul(w, key.first) || w->fusedTensor || w->operandList[1] != head->operandList[1] ||
            producerOf(w->operandList[0]) || producerOf(head->operandList[0]) || (m && w->operandList[0] != idW[0]->operandList[0]))
          continue;
        U[m] = Chain(c.begin() + 1, c.end());
        idHead[m] = head; idW[m] = w;
        if (m == 0) { addendAutos = autos; addend = head->operandList[0]; }
      }
      allU = !U[m].empty() && (m == 0 || (idHead[m] != nullptr) == (idHead[0] != nullptr));   // the identity step: all groups or none, as U
    }
    for (size_t r = 0; r < R && allU; ++r)   // the rotated source is read by the M chains and nothing else
      for (Instruction *reader : rd[addendAutos[r]->OutputOperand]) {
        bool mine = false;
        for (size_t m = 0; m < M; ++m) mine = mine || reader == U[m][r];
        allU = allU && mine;
      }
    if (!allU) addend = 0;
    const bool identity = addend && idHead[0];
    Instruction *c = mem[0].first;
    std::vector<std::vector<AddrType>> ys;
    std::vector<uint32_t> gs;
    for (size_t r = 0; r < R; ++r) {
      ys.insert(ys.end(), mem[r].first->ipY.begin(), mem[r].first->ipY.end());
      gs.push_back(mem[r].second[0]->galois);
      absorb(c, mem[r].first);
      for (Instruction *a : mem[r].second) absorb(c, a);
      for (size_t m = 0; m < M; ++m) {
        for (size_t k = 0; k < 2; ++k) absorb(c, S[m][k][r]);
        if (addend) absorb(c, U[m][r]);
      }
      if (addend) absorb(c, addendAutos[r]);
    }
    std::vector<AddrType> outs;
    for (size_t m = 0; m < M; ++m) {
      outs.push_back(S[m][0].back()->OutputOperand);
      outs.push_back(S[m][1].back()->OutputOperand);
      if (addend) outs.push_back(U[m].back()->OutputOperand);
      if (identity) {
        outs.push_back(idW[m]->OutputOperand);
        c->ipLinIdPt.push_back(idHead[m]->operandList[1]);
        c->ipLinAddend1 = idW[m]->operandList[0];
        absorb(c, idHead[m]);
        absorb(c, idW[m]);
      }
    }
    c->ipLinPt = pt;
    c->ipLinAddend = addend;
    carry(c, key.second, ys, gs, outs);
  }
}

// (6s) sum of rotations of DIFFERENT ciphertexts (hrotsum): key-product records of (6) with one modulus whose digits are all automorphisms, one
//      element per record, of materialised digits nothing else reads — the digit lists DIFFER between the records, which is what rotationGroups
//      does not group — and whose outputs k = 0, 1 are read only by ONE chain of EWE_ADD records each that adds one record's output k per link,
//      S_k = sum_c acc_{c,k}, merge WITH the two chains into one record: hm_inner_product_rotsum sums the raw products of every ciphertext in
//      registers and stores S_0, S_1 only.  If a third ADD chain (the Q limbs: U = sum_c sigma_c(c0 of ciphertext c)) adds automorphisms by the
//      same elements, in the same order, each of its own source, it joins as the record's addend output.  Never written: the rotated digits, the
//      2G per-ciphertext sums, the partial sums, the rotated c0's.  The first key-product record in stage order carries the merged one; it moves
//      to where the last link of S_0, S_1 stood: every ciphertext's digits are older, every reader of S_k and U comes after the chains' ends.
//      Initial sums (hbsgs with the identity step): ONE trailing ADD per chain whose other operand is no candidate record's output, written
//      before the carrying record, joins as the value the sum starts from (all chains or none; then one record alone may merge too).
//      Reads: the key-product records of (6).  Sets on the carrying record: ipX, ipSumX (every ciphertext's unrotated digits), ipY, ipHoistG,
//      ipSumAddend, ipSumInit, ipSumAddendInit, OutputOperand, extraOutputs.
void Arch::Planner::sumOfRotations() {
  Readers rd = readers();
  RotationGroups found = rotationGroups(rd);
  struct Member { Instruction *ip; std::vector<Instruction *> autos; std::vector<AddrType> digits; };
  std::map<Instruction *, Member> candidates;   // (looked up only)
  for (const DigitsKey &key : found.order)
    for (auto &m : found.members[key]) candidates[m.first] = Member{m.first, m.second, key.second};
  Placement place(st);
  // the one live reader of `a`, if it is an ADD of this modulus that reads `a` once; `other`: what it adds to `a`
  auto addOf = [&](AddrType a, uint32_t mod, AddrType &other) -> Instruction * {
    Instruction *l = soleReader(rd, a, EWE_ADD, mod);
    if (!l || (l->operandList[0] == a) == (l->operandList[2] == a)) return nullptr;
    other = l->operandList[0] == a ? l->operandList[2] : l->operandList[0];
    return l;
  };
  std::vector<Instruction *> order;
  for (auto &s : st)
    for (Instruction *i : s.ins)
      if (candidates.count(i)) order.push_back(i);
  std::set<Instruction *> taken;
  for (Instruction *c : order) {
    if (taken.count(c)) continue;
    const uint32_t mod = c->mod_id;
    // S_0: link by link, the running sum plus the output 0 of a further candidate record
    std::vector<Instruction *> mem = {c}, S[2];
    AddrType end[3] = {c->OutputOperand, c->extraOutputs[0], 0};   // where the chains S_0, S_1, U end
    for (AddrType &sum = end[0]; mem.size() < HM_IP_ROTSUM_MAX_CT;) {
      AddrType other = 0;
      Instruction *l = addOf(sum, mod, other), *ip = l ? producerOf(other) : nullptr;
      if (!ip || !candidates.count(ip) || taken.count(ip) || ip->mod_id != mod || ip->OutputOperand != other || !onlyReader(rd, other, l) ||
          ip->ipX.size() != c->ipX.size() || std::find(mem.begin(), mem.end(), ip) != mem.end())
        break;
      mem.push_back(ip);
      S[0].push_back(l);
      sum = l->OutputOperand;
    }
    const size_t G = mem.size();
    // the initial sums: ONE trailing ADD per chain whose other operand is no candidate record's output (hbsgs with the identity step: group 0's
    // sums S_{0,k}, which were never brought down).  `init` = that operand
    auto trailing = [&](AddrType sum, AddrType &init) -> Instruction * {
      Instruction *l = addOf(sum, mod, init), *w = l ? producerOf(init) : nullptr;
      return l && !(w && candidates.count(w)) ? l : nullptr;
    };
    AddrType init[3] = {0, 0, 0};
    Instruction *tail[3] = {G < HM_IP_ROTSUM_MAX_CT ? trailing(end[0], init[0]) : nullptr, nullptr, nullptr};
    if (G < 2 && !tail[0]) continue;
    // S_1: the same records in the same order
    bool ok = true;
    for (AddrType &sum = end[1]; ok && S[1].size() + 1 < G;) {
      AddrType other = 0;
      Instruction *l = addOf(sum, mod, other), *ip = mem[S[1].size() + 1];
      ok = l && other == ip->extraOutputs[0] && onlyReader(rd, other, l);
      if (ok) { S[1].push_back(l); sum = l->OutputOperand; }
    }
    if (!ok) continue;
    if (tail[0]) tail[1] = trailing(end[1], init[1]);
    if (tail[0] && !tail[1]) {   // initial sums for both or for none
      if (G < 2) continue;
      tail[0] = nullptr;
    }
    // where the merged record goes: the place of the last key product or link of S_0, S_1.  Every limb's record then stands in the stage of
    // S_1's last link, so that the records with and without an addend share a launch
    Instruction *last = c;
    for (Instruction *i : mem) if (place.after(i, last)) last = i;
    for (auto &chain : S) for (Instruction *i : chain) if (place.after(i, last)) last = i;
    for (int k = 0; k < 2 && tail[0]; ++k) {
      if (place.after(tail[k], last)) last = tail[k];
      if (Instruction *w = producerOf(init[k])) ok = ok && !place.after(w, c);   // written before anything of the merged record
    }
    if (!ok) continue;
    // U: an ADD chain over automorphisms by the records' elements, in their order, each of its own source (written, if at all, before that
    // place) and read by its link only
    std::vector<Instruction *> U, addendAutos;
    bool foundU = false;
    for (auto &s : st) {
      for (Instruction *a0 : s.ins) {
        if (!live(a0) || a0->ops != AUTO || a0->mod_id != mod || a0->galois != candidates[c].autos[0]->galois || rd[a0->OutputOperand].size() != 1) continue;
        if (std::find(candidates[c].autos.begin(), candidates[c].autos.end(), a0) != candidates[c].autos.end()) continue;
        std::vector<Instruction *> links, autos = {a0};
        for (AddrType sum = a0->OutputOperand; autos.size() < G;) {
          AddrType other = 0;
          Instruction *l = addOf(sum, mod, other), *a = l ? producerOf(other) : nullptr;
          if (!a || !live(a) || a->ops != AUTO || a->mod_id != mod || a->galois != candidates[mem[autos.size()]].autos[0]->galois || !onlyReader(rd, other, l))
            break;
          if (Instruction *w = producerOf(a->operandList[0])) if (place.after(w, last)) break;
          autos.push_back(a);
          links.push_back(l);
          sum = l->OutputOperand;
        }
        if (Instruction *w = producerOf(a0->operandList[0])) if (place.after(w, last)) continue;
        if (autos.size() != G) continue;
        end[2] = links.empty() ? a0->OutputOperand : links.back()->OutputOperand;
        if (tail[0]) {   // with initial sums the addend sum has one too, or does not join
          tail[2] = trailing(end[2], init[2]);
          Instruction *w = tail[2] ? producerOf(init[2]) : nullptr;
          if (!tail[2] || (w && place.after(w, c))) continue;
        } else if (G < 2) continue;
        U = links; addendAutos = autos; foundU = true;
        break;
      }
      if (foundU) break;
    }
    std::vector<std::vector<AddrType>> xs, ys;
    std::vector<uint32_t> gs;
    std::vector<AddrType> addends;
    for (size_t g = 0; g < G; ++g) {
      const Member &m = candidates[mem[g]];
      xs.push_back(m.digits);
      ys.insert(ys.end(), m.ip->ipY.begin(), m.ip->ipY.end());
      gs.push_back(m.autos[0]->galois);
      taken.insert(m.ip);
      absorb(c, m.ip);
      for (Instruction *a : m.autos) absorb(c, a);
      if (g) { absorb(c, S[0][g - 1]); absorb(c, S[1][g - 1]); }
      if (foundU) { addends.push_back(addendAutos[g]->operandList[0]); absorb(c, addendAutos[g]); if (g) absorb(c, U[g - 1]); }
    }
    for (int k = 0; k < 3 && tail[0]; ++k)
      if (tail[k]) { end[k] = tail[k]->OutputOperand; absorb(c, tail[k]); }
    if (tail[0]) { c->ipSumInit = {init[0], init[1]}; c->ipSumAddendInit = tail[2] ? init[2] : 0; }
    std::vector<AddrType> outs = {end[0], end[1]};
    if (foundU) outs.push_back(end[2]);
    c->ipSumX = xs;
    c->ipSumAddend = addends;
    carry(c, xs[0], ys, gs, outs);
    place.moveTo(c, last);
  }
}

// (6h) hoisted rotations (hrotate_hoisted): two-key inner-product records whose digits are all automorphisms (one element per record) of the SAME
//      materialised digits, read by nothing else, merge into ONE record per (modulus, digit list): hm_inner_product_hoisted reads the digits once
//      for every rotation and gathers the key / scatters the output at the automorphism's destination; the automorphisms are never written.
//      The first record in stage order carries the merged one: every reader of any rotation's output comes after it.
//      Reads: the key-product records of (6).  Sets on the carrying record: ipX (the unrotated digits), ipY, ipHoistG, OutputOperand, extraOutputs.
void Arch::Planner::hoist() {
  Readers rd = readers();
  RotationGroups found = rotationGroups(rd);
  for (const DigitsKey &key : found.order) {
    const auto &mem = found.members[key];
    for (size_t b = 0; b < mem.size(); b += HM_IP_HOISTED_MAX_ROT) {
      const size_t e = std::min(mem.size(), b + (size_t)HM_IP_HOISTED_MAX_ROT);
      if (!distinctElements(mem, b, e)) continue;
      Instruction *c = mem[b].first;
      std::vector<AddrType> outs;
      std::vector<std::vector<AddrType>> ys;
      std::vector<uint32_t> gs;
      for (size_t m = b; m < e; ++m) {
        Instruction *i = mem[m].first;
        outs.push_back(i->OutputOperand);
        outs.insert(outs.end(), i->extraOutputs.begin(), i->extraOutputs.end());
        ys.insert(ys.end(), i->ipY.begin(), i->ipY.end());
        gs.push_back(mem[m].second[0]->galois);
        absorb(c, i);
        for (Instruction *a : mem[m].second) absorb(c, a);
      }
      carry(c, key.second, ys, gs, outs);
    }
  }
}

// (7) HPIP as SURVEY.md 8f-2 specifies it: a forward transform whose only reader is an inner-product record moves INTO that
//     record (ModUp_NTT_(j) + InnerProOut: src/Operation.cpp:190-414).  The kernel runs the digit's ROW pass and multiplies
//     its registers into both keys' accumulators; the extended digit (NTTOut_beta(j)) is never written or read back — its
//     buffer only serves the first pass as scratch.
// (8) the base conversion that produces such a digit, if nobody else reads its output, moves into the transform's first pass as well
//     (decided per digit; taken only if every transformed digit of the record allows it).
//     Reads: the key-product records of (6), not the hoisted ones of (6h); fusedSubScale (4).  Sets on every such record: ipSrc, ipCoeff; (8):
//     ipConvIn, ipConvMods.
void Arch::Planner::transformTimesKey() {
  Readers rd = readers();
  for (auto &s : st)
    for (Instruction *ip : s.ins) {
      if (!isKeyProduct(*ip) || dead.count(ip) || !ip->ipHoistG.empty()) continue;   // (6h): its digits stay materialised
      ip->ipSrc = ip->ipX;
      ip->ipCoeff.assign(ip->ipX.size(), 0);
      std::vector<Instruction *> conv(ip->ipX.size(), nullptr);
      // widest digit the fused conversion + first pass takes (0: none at this ring size); config key fuse_bconv_max_in caps it below what the
      // back-end offers (A/B runs: 15 = the plan of rounds 3-5, where wider digits kept a conversion launch of their own)
      // (default: the widest digit for which the fused form measured faster at this ring size, cap_bconv_col_pref_in)
      const uint32_t maxConvIn = std::min<uint32_t>(cap("cap_bconv_col_max_in"), A.config->getValueOr("fuse_bconv_max_in", cap("cap_bconv_col_pref_in")));
      bool allConv = A.fuseBconv && (A.world_ == 1 || A.shardFused || A.shardGather) && maxConvIn != 0;
      for (size_t j = 0; j < ip->ipX.size(); ++j) {
        Instruction *t = producerOf(ip->ipX[j]);
        if (!t) continue;
        if (t->ops != NTT || t->passthrough || t->fusedSubScale || dead.count(t) || t->mod_id != ip->mod_id) continue;
        if (!onlyReader(rd, ip->ipX[j], ip)) continue;
        ip->ipSrc[j] = t->operandList[0];
        ip->ipCoeff[j] = 1;
        ip->refInstructions += t->refInstructions;
        dead.insert(t);
        // (8) is the transform's input a conversion output that nobody else reads?
        Instruction *cv = producerOf(t->operandList[0]);
        if (cv && cv->ops == BCONV_STEP2 && !dead.count(cv) && onlyReader(rd, t->operandList[0], t) && cv->operandList.size() - 1 <= maxConvIn &&
            cv->mod_id == ip->mod_id)
          conv[j] = cv;
        else allConv = false;
      }
      if (allConv && transformsInside(*ip)) {
        ip->ipConvIn.assign(ip->ipX.size(), {});
        ip->ipConvMods.assign(ip->ipX.size(), {});
        for (size_t j = 0; j < ip->ipX.size(); ++j) {
          if (!conv[j]) continue;
          ip->ipConvIn[j].assign(conv[j]->operandList.begin(), conv[j]->operandList.end() - 1);
          ip->ipConvMods[j] = conv[j]->inMods;
          ip->refInstructions += conv[j]->refInstructions * bconvPorts();
          dead.insert(conv[j]);
        }
      }
    }
}

// (7b, round 5) an inner-product record (HPIP form) whose outputs are read by inverse transforms and nothing else — the special limbs of
//      the key-switch sum (ModDownINTTOut_Key(k)) and, with (4c), the last Q limb (the rescale residue's INTT) — hands them over as the
//      FIRST pass of that inverse transform: a ROW pass over the 16 rows of the limb-poly the workgroup has just accumulated (the forward
//      ROW pass's last round and the inverse ROW pass's first are the same round, so the pass runs from the registers).  The kernel stores
//      the pass's hand-off into the INTT's output limb, the INTT record keeps its COL pass (hm_ntt_second_pass, with its scale), and the
//      evaluation-form sums of those limbs (InnerProduceOut_Key{k}[0 .. alpha)) are never written or read back.
//      Reads: ipCoeff (7).  Sets: ipInvOut, OutputOperand / extraOutputs on the key product; secondOnly, operandList[0] on the inverse transforms.
void Arch::Planner::keyProductInverseOut() {
  Readers rd = readers();
  for (auto &s : st)
    for (Instruction *ip : s.ins) {
      if (!isKeyProduct(*ip) || dead.count(ip) || ip->ipInvOut) continue;
      if (!transformsInside(*ip)) continue;   // the fused transform x key kernel only
      std::vector<AddrType *> outs = {&ip->OutputOperand};
      for (AddrType &o : ip->extraOutputs) outs.push_back(&o);
      std::vector<Instruction *> inv;
      for (AddrType *o : outs) {
        auto &r = rd[*o];
        if (r.size() != 1 || r[0]->ops != INTT || dead.count(r[0]) || r[0]->mod_id != ip->mod_id || r[0]->secondOnly || r[0]->operandList[0] != *o) break;
        inv.push_back(r[0]);
      }
      if (inv.size() != outs.size()) continue;
      for (size_t k = 0; k < outs.size(); ++k) {
        *outs[k] = inv[k]->OutputOperand;                      // the hand-off lands where the inverse transform finishes in place
        inv[k]->operandList[0] = inv[k]->OutputOperand;
        inv[k]->secondOnly = true;
      }
      ip->ipInvOut = true;
    }
}

// (9, round 4) the ModDown side of (8): a fused forward transform (ModDowNTT + ModDownSub [+ rescale]) whose input is a P -> Q conversion
//     output that nobody else reads takes the conversion into its first pass (src/Operation.cpp:489-590): ModdownBConvOut_Key(k) is
//     never written or read back.  The last limb of a key keeps its conversion: the rescale residue is formed from it element-wise (4c).
//     Reads: fusedSubScale (4), fMix (4b).  Sets on the transform: fConvIn, fConvMods.
void Arch::Planner::modDownConversion() {
  const uint32_t maxMixIn = cap("cap_bconv_col_max_in_mix");
  Readers rd = readers();
  for (auto &s : st)
    for (Instruction *t : s.ins) {
      if (t->ops != NTT || !t->fusedSubScale || t->passthrough || t->fMinuendB || dead.count(t)) continue;   // (a product minuend: not with a conversion)
      Instruction *cv = producerOf(t->operandList[0]);
      if (!cv || cv->ops != BCONV_STEP2 || dead.count(cv) || cv->mod_id != t->mod_id) continue;
      if (!onlyReader(rd, t->operandList[0], t) || cv->operandList.size() - 1 > (t->fMix ? maxMixIn : cap("cap_bconv_col_max_in"))) continue;
      t->fConvIn.assign(cv->operandList.begin(), cv->operandList.end() - 1);
      t->fConvMods = cv->inMods;
      t->refInstructions += cv->refInstructions * bconvPorts();
      dead.insert(cv);
    }
}

// (10, round 4) r = (wa - conv_last) * kT [+ wb] (4c) directly behind the conversion that produces conv_last: the one-limb element-wise
//      launch becomes the conversion kernel's epilogue (hm_bconv_desc::sub_from).
//      Reads: the SUB_SCALE[_ADD] record of (4c).  Sets on the conversion: fusedEpi, fSubFrom, fAdd, hasConstant, constant, OutputOperand, refExtra;
//      moves it to the element-wise record's place in the stage list.
void Arch::Planner::conversionEpilogue() {
  Readers rd = readers();
  for (auto &s : st)
    for (size_t ei = 0; ei < s.ins.size(); ++ei) {
      Instruction *e = s.ins[ei];
      if (e->ops != MULT || dead.count(e) || (e->opcode != EWE_SUB_SCALE && e->opcode != EWE_SUB_SCALE_ADD)) continue;
      Instruction *cv = producerOf(e->operandList[2]);
      if (!cv || cv->ops != BCONV_STEP2 || dead.count(cv) || cv->fusedEpi || cv->mod_id != e->mod_id || rd[e->operandList[2]].size() != 1) continue;
      cv->fusedEpi = true;
      cv->fSubFrom = e->operandList[0];
      cv->fAdd = e->opcode == EWE_SUB_SCALE_ADD ? e->operandList[3] : 0;
      cv->hasConstant = true;
      cv->constant = e->constant;
      cv->OutputOperand = e->OutputOperand;
      cv->refExtra += e->refInstructions;   // (a conversion's own count is scaled by the MAC ports at launch time, the epilogue's is not)
      producer[cv->OutputOperand] = cv;
      // the conversion now reads what e read (the inverse transforms of 4c, queued in e's stage): it takes e's place in the stage list,
      // which stays a topological order
      for (auto &s2 : st) s2.ins.erase(std::remove(s2.ins.begin(), s2.ins.end(), cv), s2.ins.end());
      std::replace(s.ins.begin(), s.ins.end(), e, cv);
      dead.insert(e);
    }
}

// (11, round 5) split-30 packed conversion inputs.  A limb-poly that an inverse transform writes and that nothing but base conversions read
//      (as a conversion INPUT: a separate conversion, a conversion inside a transform x key record or inside a fused transform) is
//      stored packed; a conversion takes packed inputs only if all of them are.
//      Reads: ipConvIn (8), fConvIn (9), fMix (4b), secondOnly (7b), fusedEpi (10).  Sets: packedOut on inverse transforms, inPacked / ipConvPacked
//      on the records that convert.
void Arch::Planner::packConversionInputs() {
  struct Conv { std::vector<AddrType> in; Instruction *ins; size_t digit; };   // digit: index into ipConvIn, kNoDigit = the record's own conversion
  std::vector<Conv> convs;
  std::map<AddrType, int> otherReads;   // reads of an address that are not a conversion input
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (dead.count(i)) continue;
      size_t first = convs.size();
      for (const Read &r : recordReads(*i)) {
        if (!r.loaded()) continue;                     // a replaced input is read by nobody
        if (r.role == Role::SecondPassIn) continue;    // (7b) its one operand is its own output: the in-place second pass is no other reader of it
        const bool plainConv = r.role == Role::ConvIn && !(i->ops != BCONV_STEP2 && r.digit == kNoDigit && i->fMix);   // (the fused conversion with the mix prologue takes plain inputs)
        if (!plainConv) { otherReads[r.addr]++; continue; }
        size_t c = first;
        while (c < convs.size() && convs[c].digit != r.digit) ++c;
        if (c == convs.size()) convs.push_back(Conv{{}, i, r.digit});
        convs[c].in.push_back(r.addr);
      }
    }
  std::set<AddrType> cand;
  for (auto &s : st)
    for (Instruction *x : s.ins)
      if (x->ops == INTT && !dead.count(x) && !otherReads.count(x->OutputOperand)) cand.insert(x->OutputOperand);
  for (bool changed = true; changed;) {   // a conversion with one plain input keeps all of its inputs plain
    changed = false;
    for (const Conv &cv : convs) {
      bool all = true;
      for (AddrType a : cv.in) all &= cand.count(a) != 0;
      if (all) continue;
      for (AddrType a : cv.in) changed |= cand.erase(a) != 0;
    }
  }
  std::set<AddrType> read;
  for (const Conv &cv : convs) {
    if (cv.in.empty() || !cand.count(cv.in[0])) continue;
    if (cv.digit != kNoDigit) { cv.ins->ipConvPacked.resize(cv.ins->ipConvIn.size(), 0); cv.ins->ipConvPacked[cv.digit] = 1; }
    else cv.ins->inPacked = true;
    read.insert(cv.in.begin(), cv.in.end());
  }
  for (auto &s : st)
    for (Instruction *x : s.ins)
      if (x->ops == INTT && !dead.count(x) && read.count(x->OutputOperand)) x->packedOut = true;
}

// (12) round 6: an automorphism whose output is read ONLY as the input of inverse transforms, as the addend of fused forward transforms and / or as
//      the evaluation-form digits of transform x key records folds into those readers (hm_ntt_desc.in_galois, hm_ntt_fused_desc.addend_galois,
//      hm_ntt_ip_desc.x_galois): the index map takes aligned blocks to aligned blocks, so a kernel gathers through it with its own 16-byte loads,
//      and AUTOOutput is never written or read back.  hrotate: AUTO_Key(1) -> ModUp_INTT + the key product's own digits, AUTO_Key(0) -> the final
//      add inside ModDowNTT's epilogue: 6 -> 5 launches, 140 limb-polys less traffic.  Config key fuse_auto (default 1).
//      The key product takes ONE Galois element per launch: its records fold only if every evaluation-form digit of every such record of the op
//      is the output of a foldable automorphism by the same element.  Sharded plans fold the same way: a limb-poly's transforms and key product run on
//      the rank that owns the limb, where the automorphism's source limb lives too.
//      Reads: fusedSubScale / fAddend (4), fMix (4b), ipHoistG (6h), ipSrc / ipCoeff (7), ipConvIn (8), secondOnly (7b), fConvIn (9).  Sets: inGalois +
//      operandList[0] on inverse transforms, fAddendGalois + fAddend on fused forward transforms, ipXGalois + ipX / ipSrc on key products.
void Arch::Planner::foldAutomorphisms() {
  enum Fold { NONE, INTT_IN, ADDEND, OWN_DIGIT };   // how a reader can read through the automorphism (NONE: it cannot)
  struct Reader { Instruction *ins; Fold fold; size_t digit; };
  std::map<AddrType, std::vector<Reader>> readers;
  std::vector<Reader> ownDigits;
  for (auto &s : st)
    for (Instruction *i : s.ins) {
      if (dead.count(i)) continue;
      for (const Read &r : recordReads(*i)) {
        Fold f = NONE;
        // a transform x key record reads its own digits in evaluation form, a plain inner-product record (no digit transformed inside) all of them
        // (any plan: a limb-poly's key product runs on the rank that owns the limb, and so does the automorphism's source limb)
        if (r.role == Role::IpDigit && !i->ipXGalois && i->ipHoistG.empty()) f = OWN_DIGIT;
        else if (r.role == Role::InttIn && !i->inGalois && !i->inMulB) f = INTT_IN;
        else if (r.role == Role::Addend && i->ops == NTT && !i->fMix && i->fConvIn.empty() && !i->fAddendGalois && !i->fMinuendB) f = ADDEND;
        readers[r.addr].push_back({i, f, r.digit});
        if (f == OWN_DIGIT) ownDigits.push_back({i, f, r.digit});
      }
    }
  // (the readers will read the automorphism's SOURCE, and later than the automorphism did: nothing may write that source from the automorphism's
  // stage on — the reference's operations never write their inputs; a program that does keeps its launch).  Outputs only: the first-pass scratch
  // of a transformed digit is the buffer of a forward transform's output, which is no automorphism's source.
  std::map<AddrType, size_t> lastWrite;
  for (size_t si = 0; si < st.size(); ++si)
    for (Instruction *i : st[si].ins) {
      if (dead.count(i)) continue;
      for (const Write &w : recordWrites(*i))
        if (w.role == WriteRole::Output) lastWrite[w.addr] = si;
    }
  std::map<AddrType, Instruction *> cand;   // output address -> the automorphism that every reader can read through
  bool anyOwn = false;
  for (size_t si = 0; si < st.size(); ++si)
    for (Instruction *a : st[si].ins) {
      if (a->ops != AUTO || dead.count(a) || a->galois <= 1) continue;
      { auto w = lastWrite.find(a->operandList[0]); if (w != lastWrite.end() && w->second >= si) continue; }
      auto r = readers.find(a->OutputOperand);
      if (r == readers.end() || r->second.empty()) continue;   // nobody reads it inside the op: a result
      bool ok = true;
      for (const Reader &x : r->second) ok &= x.fold != NONE && x.ins->mod_id == a->mod_id && x.ins->OutputOperand != a->operandList[0];
      if (!ok) continue;
      cand[a->OutputOperand] = a;
      for (const Reader &x : r->second) anyOwn |= x.fold == OWN_DIGIT;
    }
  if (anyOwn) {   // one Galois element per key-product launch
    uint32_t g0 = 0;
    bool uniform = true;
    for (const Reader &x : ownDigits) {
      auto c = cand.find((x.ins->ipSrc.empty() ? x.ins->ipX : x.ins->ipSrc)[x.digit]);
      if (c == cand.end() || (g0 && c->second->galois != g0)) { uniform = false; break; }
      g0 = c->second->galois;
    }
    if (!uniform)
      for (auto it = cand.begin(); it != cand.end();) {
        bool own = false;
        for (const Reader &x : readers[it->first]) own |= x.fold == OWN_DIGIT;
        it = own ? cand.erase(it) : std::next(it);
      }
  }
  for (auto &kv : cand) {
    Instruction *a = kv.second;
    auto &rd = readers[kv.first];
    for (const Reader &x : rd) {
      if (x.fold == INTT_IN) { x.ins->operandList[0] = a->operandList[0]; x.ins->inGalois = a->galois; }
      else if (x.fold == ADDEND) { x.ins->fAddend = a->operandList[0]; x.ins->fAddendGalois = a->galois; }
      else {
        x.ins->ipX[x.digit] = a->operandList[0];
        if (!x.ins->ipSrc.empty()) x.ins->ipSrc[x.digit] = a->operandList[0];
        x.ins->ipXGalois = a->galois;
      }
    }
    rd.front().ins->refInstructions += a->refInstructions;
    dead.insert(a);
  }
}

// drop dead instructions and empty stages; upstream instructions of eliminated pass-through records are
// accounted on the first surviving instruction so that the retired total still matches getTotalIns()
void Arch::Planner::sweep() {
  unsigned long long orphan = 0;
  std::vector<Stage> keep;
  for (auto &s : st) {
    Stage t = s;
    t.ins.clear();
    for (Instruction *i : s.ins) {
      if (!dead.count(i)) t.ins.push_back(i);
      else if (i->passthrough) orphan += i->refInstructions;
    }
    if (!t.ins.empty()) keep.push_back(t);
  }
  if (!keep.empty()) keep[0].ins[0]->refInstructions += orphan;
  st.swap(keep);
}
