// hm_bconv.inl — the base conversion's entry points (included by hm_backend.hip): hm_bconv, hm_bconv_batch, hm_bconv_col, hm_bconv_consts and
// the fused conversion + first transform pass (bconv_col_launch).  Each is argument checks, a plan (hm_bconv_plan.h: pure, also compiled and
// tested on the CPU), the problem records, then uploads and launches.

// conversion + first transform pass as a call of its own, on a range of column tiles: what a rank runs on its column slice between the two
// transposed-domain exchanges (hm_limbs_to_colslices -> hm_bconv_col -> hm_colslices_to_limbs -> hm_ntt_inner_product with x_is_coeff = 2)
extern "C" hm_status hm_bconv_col(hm_ctx *c, const hm_bconv_desc *descs, uint32_t n_desc, uint32_t tile0, uint32_t n_tiles) {
  if (!c) return HM_ERR_ARG;
  HM_TABLE_CALL(c);
  if (!descs || n_desc == 0) return fail(c, HM_ERR_ARG, "hm_bconv_col: no problems");
  for (uint32_t k = 0; k < n_desc; ++k)
    if (descs[k].sub_from) return fail(c, HM_ERR_UNSUPPORTED, "hm_bconv_col: no epilogue on a fused conversion");
  return bconv_col_launch(c, descs, n_desc, nullptr, tile0, n_tiles);
}

extern "C" hm_status hm_bconv_consts(hm_ctx *c, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids,
                                     uint32_t n_out, uint64_t *qhat_inv, uint64_t *table) {
  if (!c) return HM_ERR_ARG;
  if (!in_ids || n_in == 0 || (n_out && !out_ids)) return fail(c, HM_ERR_ARG, "hm_bconv_consts: bad basis");
  hm_status st;
  if ((st = check_mods(c, "hm_bconv_consts", in_ids, n_in)) || (n_out && (st = check_mods(c, "hm_bconv_consts", out_ids, n_out))))
    return st;
  std::vector<uint64_t> qh(n_in), tb((size_t)n_in * std::max<uint32_t>(n_out, 1));
  c->P.bconv_consts(in_ids, n_in, out_ids, n_out, qh.data(), tb.data());
  if (qhat_inv) memcpy(qhat_inv, qh.data(), 8ull * n_in);
  if (table && n_out) memcpy(table, tb.data(), 8ull * n_in * n_out);
  return HM_OK;
}

// What hm_bconv_batch ("hm_bconv") and the fused conversion check of every descriptor.  `max_in`: the widest input basis the caller's kernels take
// (`wide` / `note`: how the caller reports a wider one)
static hm_status check_bconv_desc(hm_ctx *c, const char *what, const hm_bconv_desc &d, uint32_t max_in, hm_status wide = HM_ERR_ARG, const char *note = "") {
  if (d.n_in == 0 || d.n_in > max_in) return fail(c, wide, "%s: n_in %u not in [1,%u]%s", what, d.n_in, max_in, note);
  if (d.n_out == 0 || d.n_out > HM_BCONV_MAX_OUT) return fail(c, HM_ERR_ARG, "%s: n_out %u not in [1,%d]", what, d.n_out, HM_BCONV_MAX_OUT);
  hm_status st;
  if ((st = check_limbs(c, what, d.in_limbs, d.n_in)) || (st = check_limbs(c, what, d.out_limbs, d.n_out)) ||
      (st = check_mods(c, what, d.in_ids, d.n_in)) || (st = check_mods(c, what, d.out_ids, d.n_out)))
    return st;
  for (uint32_t i = 0; i < d.n_in; ++i)
    for (uint32_t t = 0; t < d.n_out; ++t)
      if (d.in_ids[i] == d.out_ids[t]) return fail(c, HM_ERR_ARG, "%s: modulus %u is in both bases", what, d.in_ids[i]);
  return HM_OK;
}
static std::vector<HmBconvShape> bconv_shapes(const hm_bconv_desc *descs, uint32_t n_desc) {
  std::vector<HmBconvShape> s(n_desc);
  for (uint32_t pi = 0; pi < n_desc; ++pi) s[pi] = HmBconvShape{descs[pi].n_in, descs[pi].n_out, descs[pi].in_packed != 0};
  return s;
}

// The device table of a conversion for the kernel width kn (hm_bconv_table_words), cached per (input basis, output basis, kernel width); built and
// uploaded on first use
static hm_status bconv_table(hm_ctx *c, const hm_bconv_desc &d, uint32_t kn, const uint64_t **table) {
  std::vector<uint32_t> key;
  key.push_back(d.n_in | (kn != d.n_in ? kn << 16 : 0u));
  key.insert(key.end(), d.in_ids, d.in_ids + d.n_in);
  key.insert(key.end(), d.out_ids, d.out_ids + d.n_out);
  auto it = c->bconv_tables.find(key);
  if (it == c->bconv_tables.end()) {
    const std::vector<uint64_t> tt = hm_bconv_table_words(c->P, d.in_ids, d.n_in, d.out_ids, d.n_out, kn);
    uint64_t *dev = nullptr;
    HM_HIP(c, hipMalloc(&dev, 8ull * tt.size()));
    HM_HIP(c, hipMemcpy(dev, tt.data(), 8ull * tt.size(), hipMemcpyHostToDevice));
    it = c->bconv_tables.emplace(key, dev).first;
  }
  *table = it->second;
  return HM_OK;
}

extern "C" hm_status hm_bconv_batch(hm_ctx *c, const hm_bconv_desc *descs, uint32_t n_desc) {
  if (!c) return HM_ERR_ARG;
  HM_TABLE_CALL(c);
  if (!descs || n_desc == 0) return fail(c, HM_ERR_ARG, "hm_bconv_batch: no problems");
  HM_HIP(c, hipSetDevice(c->device));
  const uint32_t logN = descs[0].log_len ? descs[0].log_len : c->P.logN;
  if (logN < 8 || logN > c->P.logN) return fail(c, HM_ERR_ARG, "hm_bconv: log_len %u", logN);
  hm_status st;
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    const hm_bconv_desc &d = descs[pi];
    if (!d.in || !d.out) return fail(c, HM_ERR_ARG, "hm_bconv: null buffer");
    if ((d.log_len ? d.log_len : c->P.logN) != logN) return fail(c, HM_ERR_ARG, "hm_bconv_batch: mixed log_len");
    if ((st = check_bconv_desc(c, "hm_bconv", d, HM_BCONV_MAX_IN))) return st;
    if (!d.sub_from) continue;   // epilogue out = (sub_from - conv) * k [+ add]
    if (!d.sub_k) return fail(c, HM_ERR_ARG, "hm_bconv: the epilogue needs its constants (sub_k)");
    if (d.log_len && d.log_len != c->P.logN) return fail(c, HM_ERR_UNSUPPORTED, "hm_bconv: the epilogue works on whole limb-polys");
    if ((st = check_limbs(c, "hm_bconv", d.sub_from_limbs, d.n_out)) || (st = check_limbs(c, "hm_bconv", d.add_limbs, d.n_out))) return st;
    for (uint32_t t = 0; t < d.n_out; ++t)
      if (d.sub_k[t] >= c->P.mod[d.out_ids[t]]) return fail(c, HM_ERR_ARG, "hm_bconv: sub_k[%u] is not reduced", t);
  }
  std::vector<HmBconvProb> probs(n_desc);
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    const hm_bconv_desc &d = descs[pi];
    HmBconvProb &p = probs[pi];
    const uint64_t *table = nullptr;
    if ((st = bconv_table(c, d, d.n_in, &table))) return st;
    hm_bconv_fill(p, d.in, table, d.n_in, d.in_limbs, d.n_in, d.out_limbs, d.n_out, d.in_packed != 0);
    p.out = d.out;
    if (d.sub_from) {
      std::vector<HmTw> ek(d.n_out);
      for (uint32_t t = 0; t < d.n_out; ++t) {
        ek[t] = HmTw{d.sub_k[t], hm::shoup(d.sub_k[t], c->P.mod[d.out_ids[t]])};
        p.ep_a_limb[t] = limb_at(d.sub_from_limbs, t);
        p.ep_b_limb[t] = d.add ? limb_at(d.add_limbs, t) : 0;
      }
      const void *dk = nullptr;
      if ((st = device_table(c, ek.data(), sizeof(HmTw) * ek.size(), &dk))) return st;
      p.ep_a = d.sub_from; p.ep_b = d.add; p.ep_k = static_cast<const HmTw *>(dk);
    }
  }
  // the problem records of a launch go into a device table cached by content (plans repeat)
  for (const HmBconvLaunch &l : hm_bconv_plan(bconv_shapes(descs, n_desc).data(), n_desc, logN, c->bconv_blocks)) {
    std::vector<HmBconvProb> grp;
    for (uint32_t pi : l.members) grp.push_back(probs[pi]);
    const void *dtab = nullptr;
    if ((st = device_table(c, grp.data(), sizeof(HmBconvProb) * grp.size(), &dtab))) return st;
    HmBconvArgs a;
    a.prob = static_cast<const HmBconvProb *>(dtab); a.logN = logN; a.n_prob = (uint32_t)grp.size(); a.chunk = l.chunk;
    hipLaunchKernelGGL(k_bconv_by_n_in[l.n_in], dim3(l.grid[0], l.grid[1], l.grid[2]), dim3(HM_BCONV_THREADS), 0, c->stream, a);
    HM_HIP(c, hipGetLastError());
  }
  return HM_OK;
}

// conversion + first transform pass in one kernel (see k_bconv_col).  Same descriptors as hm_bconv_batch; `out` receives the COL pass's
// hand-off of NTT(conversion), the form k_ntt_row_ip reads.  N = 2^15 or 2^16, n_in <= HM_BCOL_MAX_IN.
// tile0 / n_tiles: the column tiles (16 columns each) to work on — all of them (n_tiles = 0) or a rank's column slice (hm_bconv_col)
static hm_status bconv_col_launch(hm_ctx *c, const hm_bconv_desc *descs, uint32_t n_desc, const BcolMix *mix, uint32_t tile0, uint32_t n_tiles) {
  if (!c || !descs || n_desc == 0) return HM_ERR_ARG;
  const uint32_t allTiles = c->P.N >> HM_TL_COL;
  if (!n_tiles) { tile0 = 0; n_tiles = allTiles; }
  if (!hm_tile_range_ok(tile0, n_tiles, allTiles)) return fail(c, HM_ERR_ARG, "fused conversion: tile range [%u, %u) of %u", tile0, tile0 + n_tiles, allTiles);
  if (!hm_caps(c->P.logN).bcol_max_in) return fail(c, HM_ERR_UNSUPPORTED, "fused conversion: N = 2^15 or 2^16 only");
  HM_HIP(c, hipSetDevice(c->device));
  const HmBcolPlan plan = hm_bcol_plan(bconv_shapes(descs, n_desc).data(), n_desc, n_tiles, c->bcol_outs, c->bcol_merge != 0, mix != nullptr);
  std::vector<HmBcolWindow> win(n_desc);
  bool farApart = false;
  hm_status st;
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    const hm_bconv_desc &d = descs[pi];
    if (!d.in || !d.out || !d.in_ids || !d.out_ids) return fail(c, HM_ERR_ARG, "fused conversion: null argument");
    const uint32_t maxIn = mix ? hm_caps(c->P.logN).bcol_max_in_mix : hm_caps(c->P.logN).bcol_max_in;
    if ((st = check_bconv_desc(c, "fused conversion", d, maxIn, HM_ERR_UNSUPPORTED, mix ? " (with the mix prologue)" : ""))) return st;
    if (d.log_len && d.log_len != c->P.logN) return fail(c, HM_ERR_UNSUPPORTED, "fused conversion: whole limb-polys only");
    if (d.out != descs[0].out) return fail(c, HM_ERR_ARG, "fused conversion: one hand-off buffer per call");
    win[pi] = hm_bcol_window(d.in_limbs, d.n_in, plan.kn[pi], c->P.logN);
    if (!win[pi].fits) { farApart = true; break; }   // inputs more than 4 GiB apart: the fallback below (which checks the rest of the call)
    for (uint32_t t = 0; mix && t < d.n_out; ++t) {
      if (mix->mix_k[pi][t] >= c->P.mod[d.out_ids[t]]) return fail(c, HM_ERR_ARG, "fused conversion: mix constant [%u][%u] is not reduced", pi, t);
      if (mix->mix_limbs[pi][t] > 0xFFFFu) return fail(c, HM_ERR_ARG, "fused conversion: limb index exceeds 65535");
    }
    // (measured with the combination built: the fused ModDown conversion stays 2.5 % behind the separate one with packed inputs too —
    // profiles/r05_late_ab.txt — so the 120 instantiations it needs are not shipped)
    if (mix && d.in_packed) return fail(c, HM_ERR_UNSUPPORTED,
        "fused conversion: packed inputs and the mix prologue do not combine (convert from plain inputs)");
  }
  if (farApart) {
    // A conversion whose input limb-polys are spread over more than 4 GiB of the buffer cannot be addressed from one descriptor with 32-bit
    // offsets.  The plans of the host layer never produce one (a digit's limbs are neighbours in the pool); a caller's list that does is
    // served by the two steps the fused kernel stands for: the conversion into the hand-off limbs, then the first pass in place on them.
    if (n_tiles != allTiles) return fail(c, HM_ERR_UNSUPPORTED,
        "fused conversion on a column slice: the inputs of a conversion must lie within 4 GiB of each other");
    if ((st = hm_bconv_batch(c, descs, n_desc))) return st;
    std::vector<uint32_t> limbs, mods, ml;
    std::vector<uint64_t> mk;
    for (uint32_t pi = 0; pi < n_desc; ++pi)
      for (uint32_t t = 0; t < descs[pi].n_out; ++t) {
        limbs.push_back(limb_at(descs[pi].out_limbs, t)); mods.push_back(descs[pi].out_ids[t]);
        if (mix) { ml.push_back(mix->mix_limbs[pi][t]); mk.push_back(mix->mix_k[pi][t]); }
      }
    NttFused f;
    f.firstPassOnly = true;
    if (mix) { f.mix = mix->mix; f.mix_limbs = ml.data(); f.mix_k = mk.data(); f.minuend = descs[0].out;
        /* (marks the fused form: the first pass only reads the mix operand) */ }
    std::vector<uint64_t> ones(limbs.size(), 1);
    return ntt_common(c, "fused conversion", descs[0].out, limbs.data(), descs[0].out, limbs.data(), mods.data(), (uint32_t)limbs.size(), 0, mix ?
        ones.data() : nullptr, f);
  }
  std::vector<HmBcolProb> probs(n_desc);
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    const hm_bconv_desc &d = descs[pi];
    const uint32_t kn = plan.kn[pi];
    HmBcolProb &p = probs[pi];
    const uint64_t *table = nullptr;
    if ((st = bconv_table(c, d, kn, &table))) return st;
    hm_bconv_fill(p, d.in, table, kn, d.in_limbs, d.n_in, d.out_limbs, d.n_out, d.in_packed != 0);
    p.in_base = d.in + (size_t)win[pi].base * c->P.N;
    memcpy(p.in_limb, win[pi].limb, sizeof p.in_limb);
    memcpy(p.in_off, win[pi].off, sizeof p.in_off);
    for (uint32_t t = 0; t < d.n_out; ++t) p.out_mod[t] = d.out_ids[t];
    if (mix) {   // x = conv + k * mix before the first butterfly: constants in Shoup form, a device table cached by content
      std::vector<HmTw> mk(d.n_out);
      for (uint32_t t = 0; t < d.n_out; ++t) {
        mk[t] = hm_kconst(mix->mix_k[pi][t], c->P.mod[d.out_ids[t]]);
        p.mix_limb[t] = mix->mix_limbs[pi][t];
      }
      const void *dk = nullptr;
      if ((st = device_table(c, mk.data(), sizeof(HmTw) * mk.size(), &dk))) return st;
      p.mixk = static_cast<const HmTw *>(dk);
    }
  }
  const dim3 block((1 << HM_TL_COL) / HM_EPT);
  for (const HmBcolLaunch &l : plan.launches) {
    std::vector<HmBcolProb> grp;
    for (uint32_t pi : l.members) grp.push_back(probs[pi]);
    const void *dtab = nullptr;
    if ((st = device_table(c, grp.data(), sizeof(HmBcolProb) * grp.size(), &dtab))) return st;
    // (one hand-off buffer for the call: checked above)
    HmBcolArgs a = {static_cast<const HmBcolProb *>(dtab), descs[0].out, c->d_tw_fwd, c->P.logN, (uint32_t)grp.size(), l.groups, mix ? mix->mix : nullptr, tile0,
        l.logTiles};
    const hm_bcol_kernel kern = hm_bcol_kernel_for(l.key & 255u, c->P.logN, plan.NOUT, mix != nullptr, l.key >= 256u);
    if (!kern) return fail(c, HM_ERR_UNSUPPORTED, "fused conversion: no kernel for n_in %u at N = 2^%u", l.key, c->P.logN);
    hipLaunchKernelGGL(kern, dim3(l.grid), block, 0, c->stream, a);
    HM_HIP(c, hipGetLastError());
  }
  return HM_OK;
}

extern "C" hm_status hm_bconv(hm_ctx *c, const uint64_t *in, const uint32_t *in_limbs, const uint32_t *in_ids,
                              uint32_t n_in, uint64_t *out, const uint32_t *out_limbs, const uint32_t *out_ids,
                              uint32_t n_out) {
  hm_bconv_desc d = {in, in_limbs, in_ids, n_in, out, out_limbs, out_ids, n_out, 0};
  return hm_bconv_batch(c, &d, 1);
}
