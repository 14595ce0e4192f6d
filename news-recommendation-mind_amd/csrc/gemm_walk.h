// The persistent unit walk of the fast GEMM kernels, ONE text for gemm_fast_body (gemm_fast_impl.h) and
// gemm_split_kernel (gemm_split_impl.h): a fragment #included inside the kernel body, not a header of
// declarations (no include guard).  It is shared as text, not as a type with member functions, because
// the kernels must compile to the code they had as two copies: a walker object (state behind
// references, the unit bookkeeping behind a call) changed register allocation in every instantiation
// and measured 6-8 % slower on the 64 x 64 weight-gradient kernels.
//
// Two parts, chosen by NR_WALK_PART (defined before each #include, undefined here), so that the
// statements keep the places they had in the kernels:
//   1  needs Args g (clamp_extents applied), int gn, ntiles, units (tile columns, tiles, tiles x splits
//      of the clamped extents), bid, G (this workgroup's place in its grid), constexpr int BM, BN.
//      Leaves skip_empty, advance, kof, peek_k and the compute position cp: the workgroup's first
//      non-empty unit (the kernel has returned when there is none).
//   2  needs part 1, int tid, constexpr bool IDX_AHEAD and the loaders LA la, LB lb.  Leaves the load
//      position lp (one or two positions ahead of cp), issue and step_load, with the first position's
//      token ids fetched and its loads issued.
#if NR_WALK_PART == 1
  // first non-empty unit at or after virtual id `id` in this block's sequence (a split past a
  // device-resident K is empty), or `units`
  auto skip_empty = [&](int id, Unit& u) -> int {
    for (; id < units; id += G) {
      u = decode_unit(g, id, units, ntiles, gn, BM, BN);
      if (u.nt > 0) return id;
    }
    return units;
  };
  // cursor advance: false when the block's sequence is exhausted
  auto advance = [&](Cursor& p) -> bool {
    if (p.kt + 1 < p.u.nt) { ++p.kt; return true; }
    Unit u;
    const int nid = skip_empty(p.id + G, u);
    if (nid >= units) return false;
    p.id = nid;
    p.kt = 0;
    p.u = u;
    return true;
  };
  auto kof = [](const Cursor& p) -> int64_t { return p.u.kbeg + (int64_t)p.kt * 32; };
  auto peek_k = [&](const Cursor& p) -> int64_t {   // k of the position after p, or -1
    if (p.kt + 1 < p.u.nt) return kof(p) + 32;
    Unit u;
    return skip_empty(p.id + G, u) < units ? u.kbeg : -1;
  };

  Cursor cp;   // compute position
  cp.kt = 0;
  cp.id = skip_empty(bid, cp.u);
  if (cp.id >= units) return;

#else
  Cursor lp = cp;   // load position
  la.init(g.A, lp.u.m0, g.M, tid);
  lb.init(g.B, lp.u.n0, g.N, tid);
  auto issue = [&](const Cursor& p) {
    const int64_t k = kof(p);
    la.load(g.A, p.u.m0, g.M, k, tid);
    lb.load(g.B, p.u.n0, g.N, k, tid);
    if (IDX_AHEAD) {   // token ids of the position after p, one load ahead of its data
      const int64_t pk = peek_k(p);
      if (pk >= 0) {
        la.prefetch_idx(g.A, pk, g.K, tid);
        lb.prefetch_idx(g.B, pk, g.K, tid);
      }
    }
  };
  auto step_load = [&]() -> bool {   // move lp one position and issue its loads
    const int old = lp.id;
    if (!advance(lp)) return false;
    if (lp.id != old) {
      la.init(g.A, lp.u.m0, g.M, tid);
      lb.init(g.B, lp.u.n0, g.N, tid);
    }
    issue(lp);
    return true;
  };
  if (IDX_AHEAD) {   // the first position's ids, then its loads
    la.prefetch_idx(g.A, kof(lp), g.K, tid);
    lb.prefetch_idx(g.B, kof(lp), g.K, tid);
  }
  issue(lp);
#endif
#undef NR_WALK_PART
