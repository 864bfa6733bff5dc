// The registration loops: one alignment (exact or voxelized, by any of the exact path's routes) and a batch of alignments.
// Part of ngicp_api.hip's translation unit (included there, after ngicp_voxelmap.h).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// Registration loop
// ------------------------------------------------------------------------------------------
// start / stop: events attached to the dispatch itself (they take the kernel's own begin / end timestamps: no extra packets in
// the stream, unlike hipEventRecord before and after), or null
std::mutex& persist_mutex(int device) {  // one persistent alignment per device at a time (its grid fills the device and its blocks wait for each other)
  static std::mutex m[64];
  return m[(unsigned)device % 64u];
}

// ---- the handle's side of ngicp_route.h: the facts it contributes, and the refusals as errors ----
route::Facts route_facts(const ngicp* h, route::Caller caller, int nblocks = 1) {
  route::Facts f;
  f.caller = caller;
  f.persist = h->persist;
  f.robust = h->robust_kind != NGICP_ROBUST_NONE;
  f.prior = h->prior_set;
  f.iterating = h->p.max_iter > 0;
  f.nblocks = nblocks;
  f.pass_slots = h->pass_slots;
  f.persist_slots = h->persist_slots;
  f.max_passes = max_passes(h->p);
  return f;
}
// what the entry point refuses outright (route::kEntries), as its error
void refuse_for(const ngicp* h, route::Entry e) {
  const std::string why = route::entry_refusal(e, h->voxel_res > 0.0, h->robust_kind != NGICP_ROBUST_NONE, h->prior_set);
  if (!why.empty()) throw ArgError{NGICP_ERR_ARG, why};
}
// what the switches that are set cannot do with the handle's robust kernel or pose prior (route::refusal), as the entry's error
void refuse_route(const ngicp* h, route::Caller caller, const char* entry) {
  const std::string why = route::refusal(route::switches(), h->sw, route_facts(h, caller), entry);
  if (!why.empty()) throw ArgError{NGICP_ERR_ARG, why};
}
// the pass kernel of a caller that has one launch-per-pass route to take (the hooks, ngicp_sharded_pass)
route::Variant pass_variant(const ngicp* h, route::Caller caller, int nblocks) {
  return route::choose_route(route::switches(), h->sw, route_facts(h, caller, nblocks)).variant;
}
void fill_robust(const ngicp* h, int& kind, double& c, double& c2) {
  kind = h->robust_kind;
  c = h->robust_width;
  c2 = h->robust_width * h->robust_width;
}

// One launch of the pass kernel route::choose_route picked.  32-query batches, 2 lanes per query.  Two builds of every kernel: 3 waves per
// SIMD (129 VGPRs), and 4 (128 VGPRs, two spilled dwords, 4 blocks per CU) for grids of more than two rounds of blocks, where the launch
// is bound by how many blocks pass through the chip rather than by its slowest block.
void launch_pass(ngicp* h, const PassArgs& a, const route::Variant& v, int nblocks, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  using K = void (*)(PassArgs);
  const bool four = v.waves == 4;
  K kernel = nullptr;
  PassArgs b = a;
  unsigned grid = (unsigned)nblocks;
  switch (v.family) {
    case route::Family::Staged: {  // the staged search of ngicp_pass_st.h (round 3 experiment: exact, slower - DESIGN.md §5)
      // cells that cover the distance gate around a query's own cell (its reach box is clamped there; beyond it the shell walk takes over)
      int need = kStGrowMax;
      if (h->p.max_corr_dist < 1e30) need = (int)std::ceil(h->p.max_corr_dist / (double)a.grid.h);
      b.stage_grow = std::max(1, std::min(kStGrowMax, need));
      kernel = four ? K(k_gicp_pass_st<4>) : K(k_gicp_pass_st<3>);
      break;
    }
    case route::Family::Queue:  // a grid of resident blocks that draw their groups from a counter (round 3 experiment)
      grid = (unsigned)std::min(nblocks, h->queue_slots[four]);
      kernel = four ? K(k_gicp_queue<2, 4>) : K(k_gicp_queue<2, 3>);
      break;
    case route::Family::Walks:  // walks in global memory; fused: the solver in the tail of the launch; robust: the term weighted in its K4 leg and K3 tail
      if (v.fused) kernel = four ? K(k_gicp_pass<2, 4, true>) : K(k_gicp_pass<2, 3, true>);
      else if (v.robust) kernel = four ? K(k_gicp_pass<2, 4, false, true>) : K(k_gicp_pass<2, 3, false, true>);
      else kernel = four ? K(k_gicp_pass<2, 4>) : K(k_gicp_pass<2, 3>);
      break;
  }
  hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, start, stop, 0, b);
}

struct LoopCtx {
  PassArgs pa;
  SolveArgs sa;
  int nblocks;
};

// own_buffers false (ngicp_align_batch): slots and covariances are readied and the fields every lane shares are filled in, but none of
// the handle's single-alignment buffers is sized or referred to (the caller supplies every per-alignment pointer) and no stats field is
// written: what the getters of the last ngicp_align read stays where it is.
// with_target false (the voxelized entries on a rolling map): the target slot is not read at all - it may be empty - and
// the exact pass's target fields stay null; the voxelized loops overwrite or ignore everything else that depends on it.
void prepare_loop(ngicp* h, LoopCtx& c, bool own_buffers = true, bool with_target = true) {
  ensure_slot_ready(h, h->src, "source");
  if (with_target) ensure_slot_ready(h, h->tgt, "target");
  // lazy covariances (impl/nano_gicp_impl.hpp:163-168)
  if (h->src_covs.n != h->src.dev->n) compute_covs(h, h->src, h->src_covs, "source");
  if (with_target && h->tgt_covs.n != h->tgt.dev->n) compute_covs(h, h->tgt, h->tgt_covs, "target");
  DeviceCloud& S = *h->src.dev;
  const size_t n = S.n;
  const int nblocks = std::max(1, (S.n_batches + 3) / 4);  // one block per group of four batches
  const int max_rows = max_trace_rows(h->p);
  if (own_buffers) {
    for (int i = 0; i < 2; ++i) {
      h->tpt[i].ensure(n * sizeof(float4));
      h->mahal[i].ensure(n * 6 * sizeof(double));
    }
    h->partials.ensure((size_t)kNumSlots * nblocks * sizeof(double));
    h->grp_order.ensure((size_t)nblocks * sizeof(int));
    h->grp_order_alt.ensure((size_t)nblocks * sizeof(int));
    h->grp_cost.ensure((size_t)nblocks * sizeof(int));
    {
      // (the persistent kernel's ring of per-pass views continues behind the state: one 256-byte entry per possible pass)
      const long ring = (long)max_rows + 1;
      h->state.ensure(sizeof(LmState) + (ring <= kMaxPersistPasses ? (size_t)ring * kViewWords * sizeof(int) : 0));
    }
    if (h->trace.ensure_grew((size_t)max_rows * kTraceCols * sizeof(double))) h->trace_rows_dev = 0;  // an unfetched trace went with the old buffer
    h->sums.ensure(kPartialStride * sizeof(double));
    h->batch_far.ensure((size_t)S.n_batches + 16);
    h->gen_lines.ensure((size_t)kGenLines * kGenStride * sizeof(int));
  }

  PassArgs& a = c.pa;
  fill_robust(h, a.robust_kind, a.robust_c, a.robust_c2);
  a.qpts = S.qpts.as<float4>();
  a.batches = S.batches.as<int2>();
  a.batch_boxes = S.batch_boxes.as<float>();
  int* const order_buf[2] = {own_buffers ? h->grp_order.as<int>() : nullptr, own_buffers ? h->grp_order_alt.as<int>() : nullptr};
  int* const ctl = own_buffers ? h->order_flag.as<int>() : nullptr;  // {order flag 0, ticket, gen, order flag 1}
  int* const order_flag[2] = {ctl, ctl ? ctl + 3 : nullptr};
  a.grp_order = order_buf[h->order_sel];
  a.grp_cost = own_buffers ? h->grp_cost.as<int>() : nullptr;
  a.n_batches = S.n_batches;
  a.cov_src = covs_for(h, h->src_covs, h->src.dev);
  a.n_src = (int)n;
  if (with_target) {
    DeviceCloud& T = *h->tgt.dev;
    a.tgt = T.pts();
    a.tgt3 = T.xyz3();
    a.tgtp = T.xyzp();
    a.tgt_cell_start = T.cells();
    a.tgt_cell_box = (h->sw.cell_boxes && T.has_boxes) ? T.cell_box.as<unsigned int>() + kCellPad : nullptr;
    a.cov_tgt = covs_for(h, h->tgt_covs, h->tgt.dev);
    a.grid = T.grid;
  } else {
    a.tgt = nullptr;
    a.tgt3 = nullptr;
    a.tgtp = nullptr;
    a.tgt_cell_start = nullptr;
    a.tgt_cell_box = nullptr;
    a.cov_tgt = nullptr;
    a.grid = Grid{};
  }
  for (int i = 0; i < 2; ++i) {
    a.tpt[i] = own_buffers ? h->tpt[i].as<float4>() : nullptr;
    a.mahal[i] = own_buffers ? h->mahal[i].as<double>() : nullptr;
  }
  a.gate_sq = h->p.max_corr_dist * h->p.max_corr_dist;
  {
    float f = (float)a.gate_sq;  // may round down or overflow to inf
    if ((double)f < a.gate_sq) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    a.gate_sq_f = f;
  }
  a.batch_far = own_buffers ? h->batch_far.as<unsigned char>() : nullptr;
  a.st = own_buffers ? h->state.as<LmState>() : nullptr;
  a.partials = own_buffers ? h->partials.as<double>() : nullptr;
  a.mode = 3;
  a.dbg_stamps = nullptr;
  a.dbg_qstats = nullptr;
  a.dbg_span = nullptr;
  a.order_valid = order_flag[h->order_sel];
  a.t_first = nullptr;
  a.fused = 0;
  a.persist = 0;
  a.first_pass = 0;
  a.max_passes = 0;
  a.ticket = ctl ? ctl + 1 : nullptr;
  a.gen = own_buffers ? h->gen_lines.as<int>() : nullptr;
  {
    // rings worth staging: enough to cover the distance gate (the search never looks farther), at most kStageMaxGrow
    int need = kStageMaxGrow;
    if (with_target && h->p.max_corr_dist < 1e30) need = (int)std::ceil(h->p.max_corr_dist / (double)a.grid.h);
    a.stage_grow = h->sw.stage_grow <= 0 ? 0 : std::max(1, std::min(std::min(kStageMaxGrow, h->sw.stage_grow), need));  // 0: search straight from global memory
  }

  SolveArgs& s = c.sa;
  s.st = a.st;
  s.cfg.max_iterations = h->p.max_iter;
  s.cfg.lm_max_iterations = h->p.lm_max_iter;
  s.cfg.optimizer = h->p.optimizer;
  s.cfg.rot_eps = h->p.rot_eps;
  s.cfg.trans_eps = h->p.trans_eps;
  s.cfg.lm_init_lambda_factor = h->p.lm_init_lambda_factor;
  s.partials = a.partials;
  s.nblocks = nblocks;
  s.grp_order = order_buf[h->order_sel];
  s.grp_cost = a.grp_cost;
  s.trace = own_buffers ? h->trace.as<double>() : nullptr;
  s.max_trace_rows = max_rows;
  s.mode = 0;
  s.sums_out = nullptr;
  s.dbg_stamps = nullptr;
  s.progress_host = nullptr;
  s.final_host = nullptr;
  s.order_valid = order_flag[h->order_sel];
  s.t_first = nullptr;
  s.persist = 0;
  s.pass_honours_word = 0;
  s.serial_step = h->sw.serial_step;
  s.pass_ticks = nullptr;
  s.prior = h->prior_set ? h->prior_dev.as<double>() : nullptr;
  s.st_out = nullptr;
  s.nrows = 0;
  a.crow_in = nullptr;
  a.crow_out = nullptr;
  a.cluster_ticket = nullptr;
  a.done_flag = nullptr;
  c.nblocks = nblocks;
  if (!own_buffers) return;
  h->stats.lanes_per_query = 2;
  h->stats.voxel_size = a.grid.h;
  h->stats.grid_dims[0] = a.grid.nx;
  h->stats.grid_dims[1] = a.grid.ny;
  h->stats.grid_dims[2] = a.grid.nz;
}

void init_state_from_pose(LmState& st, const Pose& x0) {
  std::memset(&st, 0, sizeof(st));
  st.hot.x0 = x0;
  st.hot.xi = x0;
  pose_identity(st.hot.delta);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) st.xi_f[r * 4 + c] = (float)x0.R[r * 3 + c];
    st.xi_f[r * 4 + 3] = (float)x0.t[r];
  }
  std::memcpy(&st.view[kViewXi], &st.hot.xi, sizeof(Pose));
  std::memcpy(&st.view[kViewXiF], st.xi_f, sizeof(st.xi_f));
  static_assert(sizeof(Pose) == 24 * sizeof(int) && kViewXiF == 24 && sizeof(LmState::xi_f) == 12 * sizeof(int), "LmState::view layout");
  st.hot.lambda = -1.0;  // impl/lsq_registration_impl.hpp:92
  st.hot.nu = 2.0;
  for (int i = 0; i < 6; ++i) st.hot.final_H[i * 6 + i] = 1.0;
}

template <class F>
Pose pose_from_colmajor(const F m[16]) {  // (float: Isometry3d(guess.cast<double>()), impl/lsq_registration_impl.hpp:90)
  Pose p;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.R[r * 3 + c] = (double)m[c * 4 + r];
    p.t[r] = (double)m[12 + r];
  }
  return p;
}
void pose_to_colmajor_f(const Pose& p, float m[16]) {  // x0.cast<float>().matrix(), :113
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m[c * 4 + r] = (float)p.R[r * 3 + c];
    m[12 + r] = (float)p.t[r];
    m[r * 4 + 3] = 0.f;
  }
  m[15] = 1.f;
}

// ---- what every alignment shares: the host's wait on the device's progress, and what an alignment leaves on the handle ----
// One turn of the wait for the solver's published progress: give up after 30 s, otherwise yield or pause.
inline void wait_for_the_loop(ngicp* h, unsigned long& spins, double t_loop) {
  if ((++spins & (h->host_wait ? 0xfff : 0xfffff)) == 0 && now_ms() - t_loop > 30000.0) throw ArgError{NGICP_ERR_HIP, "the registration loop did not finish within 30 s"};
  if (h->host_wait) sched_yield(); else __builtin_ia32_pause();
}

// A final state image's pose, `converged`, iterations and Hessian (transposed: column-major for the caller) into the handle's fields or a
// caller's arrays; any of the last three may be null.
void store_result(const LmHot& r, float T[16], int* converged, int* nr_iterations, double* hessian) {
  pose_to_colmajor_f(r.x0, T);
  if (converged) *converged = r.converged;
  if (nr_iterations) *nr_iterations = r.nr_iterations;
  if (hessian)
    for (int rr = 0; rr < 6; ++rr)
      for (int cc = 0; cc < 6; ++cc) hessian[cc * 6 + rr] = r.final_H[rr * 6 + cc];
  if (r.lm_failed) std::fprintf(stderr, "lm not converged!!\n");  // impl/lsq_registration_impl.hpp:106
}

// The final state's results, the transformed cloud if asked for, and the statistics that do not depend on the pass kernel.
void publish_alignment(ngicp* h, const LmState& st, float loop_ms, float* aligned, size_t out_stride) {
  store_result(st.hot, h->final_T, &h->converged, &h->nr_iterations, h->final_hessian);
  h->trace_host.clear();  // fetched on demand (ngicp_get_lm_trace): a diagnostic should not cost every align a synchronous copy
  h->trace_rows_dev = (size_t)st.hot.n_trace;
  if (aligned) download_transformed(h, *h->src.dev, h->final_T, aligned, out_stride);  // K5: pcl::transformPointCloud(*input_, output, final_transformation_)
  if (st.hot.have_lin) h->hook_valid = 2;  // ngicp_get_correspondences: the correspondences of the last adopted linearisation
  ngicp_stats& s = h->stats;
  s.loop_ms = loop_ms;
  s.passes = st.hot.passes;
  s.outer_iterations = st.hot.nr_iterations + 1;
  s.lm_trials = st.hot.n_trace;
  s.search_passes = st.hot.search_passes;
  // (means over the passes that searched: a K4-only pass tests no candidate and gates nothing in)
  s.mean_candidates = st.hot.search_passes > 0 ? st.hot.cand_total / ((double)st.hot.search_passes * (double)h->src.dev->n) : 0.0;
  s.valid_fraction = st.hot.search_passes > 0 ? st.hot.valid_total / ((double)st.hot.search_passes * (double)h->src.dev->n) : 0.0;
  s.pass_ms_total = 0.0;
  s.passes_timed = 0;
}

// With profiling on: HIP events on the handle's own stream around every prof_stride-th pass launch that did work.
void sum_event_pass_times(ngicp* h, long passes) {
  if (!h->profiling) return;
  ngicp_stats& s = h->stats;
  const long timed = std::min<long>(passes, (long)h->prof_events.size() / 2);
  int counted = 0;
  for (long i = h->prof_stride / 2; i < timed; i += h->prof_stride) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->prof_events[2 * i], h->prof_events[2 * i + 1]) == hipSuccess) {
      s.pass_ms_total += ms;
      ++counted;
    }
  }
  s.passes_timed = counted;
}

// ---- one alignment, written once: the prologue, the feed and the end.  do_align and do_align_voxel bring the launches ----
struct Alignment {
  double t_begin = now_ms(), t_loop = 0.0;
  LmState st;               // the state the alignment starts from; its hot part is the final one once the loop has ended
  float loop_ms = 0.f;
  unsigned long spins = 0;  // turns of the host's wait
};

// what ngicp_align returns when the alignment fails before it has a result
void reset_results(ngicp* h) {
  h->hook_valid = 0;
  h->converged = 0;
  h->nr_iterations = 0;
  std::memcpy(h->final_T, kIdentity16, sizeof(kIdentity16));  // PCL align(): final_transformation_ = Identity before computeTransformation
}

// The state an alignment starts from, built in pinned memory and uploaded from there (max_iter <= 0: it is the final one already).
const LmState& upload_initial_state(ngicp* h, const float guess[16]) {
  LmState& st = h->pin_state[0];
  init_state_from_pose(st, pose_from_colmajor(guess));
  if (h->p.max_iter <= 0) st.hot.done = 1;
  HIP_TRY(hipMemcpyAsync(h->state.p, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
  return st;
}

// The prologue: the state upload, and where the solver publishes its progress, the final state image and the first pass's stamp.
void begin_alignment(ngicp* h, Alignment& al, const float guess[16], SolveArgs& sa, unsigned long long*& pass_t_first) {
  al.st = upload_initial_state(h, guess);
  *h->h_progress = 0;
  sa.progress_host = h->h_progress;
  sa.final_host = h->pin_final;
  sa.t_first = h->t_first.as<unsigned long long>();
  pass_t_first = h->t_first.as<unsigned long long>();
  al.t_loop = now_ms();
}

// The host feeds (pass, solve) pairs to the stream and never blocks on it inside the loop: the solver publishes its progress
// {passes done, done flag} in PINNED host memory (one system-scope store), the host keeps `depth` pairs in flight and stops
// feeding when it sees the flag.  At most `depth` pairs are enqueued in vain (they return at once: the state says done);
// round 1 polled a copied flag one chunk of four pairs behind and wasted up to eight.
// launch(i, start, stop) enqueues launch number i of at most max_launches, timed by the two events unless they are null.
template <class Launch>
void feed_alignment(ngicp* h, Alignment& al, long max_launches, Launch&& launch) {
  if (h->p.max_iter <= 0) {
    HIP_TRY(hipStreamSynchronize(h->stream));  // (max_iterations <= 0: nothing was launched; the state is the initial one)
    return;
  }
  const int depth = h->sw.chunk;
  long launched = 0;
  while (launched < max_launches) {
    const int prog = *reinterpret_cast<volatile int*>(h->h_progress);
    if (prog & kProgressDone) break;
    if (launched - (long)(prog & kProgressMask) >= depth) {  // enough in flight: wait for the device to catch up
      wait_for_the_loop(h, al.spins, al.t_loop);
      continue;
    }
    const bool timed = h->profiling && launched % h->prof_stride == h->prof_stride / 2 && (size_t)(2 * launched + 1) < h->prof_events.size();
    launch(launched, timed ? h->prof_events[2 * launched] : nullptr, timed ? h->prof_events[2 * launched + 1] : nullptr);
    ++launched;
  }
  // The solver writes the final state image into pinned memory and THEN raises the done flag (system-scope release): no copy,
  // no event, no stream synchronisation - the few launches enqueued ahead return at once behind the host's back, and whatever
  // this handle enqueues next is ordered behind them on its stream.
  for (;;) {
    const int prog = __atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE);
    if (prog & kProgressDone) break;
    if (launched >= max_launches && launched - (long)(prog & kProgressMask) <= 0) break;  // (cannot happen: the last possible pass sets done)
    wait_for_the_loop(h, al.spins, al.t_loop);
  }
  al.st.hot = *h->pin_final;
  al.loop_ms = (float)((double)(al.st.hot.t_done - al.st.hot.t_first) * 1e-5);  // 100 MHz ticks -> ms
}

// The end: the results and the statistics every alignment leaves, whatever enqueued its passes.
void end_alignment(ngicp* h, Alignment& al, float* aligned, size_t out_stride, bool event_times = true) {
  publish_alignment(h, al.st, al.loop_ms, aligned, out_stride);
  if (event_times) sum_event_pass_times(h, al.st.hot.passes);
  ngicp_stats& s = h->stats;
  s.n_src = (long long)h->src.dev->n;
  s.n_tgt = rolling_active(h) ? (long long)h->roll.n_vox : (long long)h->tgt.dev->n;  // (a rolling map has no target cloud: its voxels)
  s.host_wait_spins = (long long)al.spins;
  s.align_ms = now_ms() - al.t_begin;
}

// ---- the exact path's own decisions, routes and epilogue ----
// The optimiser's mode bits of the exact pass, and bit 32:
// whether the FIRST pass lists the region rows of every batch (later passes list for the batches that looked beyond ring 1 in the
// pass before): it pays where many queries do (100k -> 500k with DLO's settings: 22 % of the batches, scan-to-submap 0.67 -> 0.64 ms)
// and costs where few do (250k -> 2M: first pass 107 -> 72 us without).  Decided from the share of queries the previous alignment
// of this handle served through lists; yes when there was none.
void set_pass_mode(const ngicp* h, PassArgs& a) {
  a.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  if (h->prev_staged_fraction < 0.0 || h->prev_staged_fraction >= 0.12) a.mode |= 32;
}

// Where the switches leave the passes free to honour LmHot::lin_unneeded (route::honours_lin_unneeded: k_gicp_pass in its default, 4-waves,
// robust and fused builds does, the other kernels keep full passes): sets the pass's mode bit and tells the solver, so that search_passes
// counts what ran and a K4-only pass leaves the launch order alone.
void allow_k4_only_passes(const ngicp* h, LoopCtx& c, const route::Facts& f) {
  if (!route::honours_lin_unneeded(route::switches(), h->sw, f)) return;
  c.pa.mode |= 64;
  c.sa.pass_honours_word = 1;
}

// NGICP_ORDER=xcd (experiment): instead of the cost-sorted launch order, a FIXED order that hands every XCD (blocks b, b + 8, ...
// are observed to share one) a contiguous eighth of the Morton-ordered groups: each XCD's L2 then sees an eighth of the target.
// true: the order is installed and the solver leaves it alone.
bool install_xcd_order(ngicp* h, LoopCtx& c) {
  if (!route::switches().xcd_order) return false;
  const int nb = c.nblocks, per = (nb + 7) / 8;
  std::vector<int> ord((size_t)nb);
  std::vector<int> lists[8];
  for (int g = 0; g < nb; ++g) lists[std::min(7, g / per)].push_back(g);
  size_t taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int b = 0;
  for (int placed = 0; placed < nb; ++b) {  // block b belongs to XCD b % 8: the next group of that XCD's list, or of the fullest one left
    int x = b % 8;
    if (taken[x] >= lists[x].size()) {
      x = 0;
      for (int y = 1; y < 8; ++y)
        if (lists[y].size() - taken[y] > lists[x].size() - taken[x]) x = y;
    }
    ord[(size_t)placed++] = lists[x][taken[x]++];
  }
  HIP_TRY(hipMemcpyAsync(const_cast<int*>(c.pa.grp_order), ord.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int one = 1;
  HIP_TRY(hipMemcpy(const_cast<int*>(c.pa.order_valid), &one, sizeof(int), hipMemcpyHostToDevice));
  c.sa.grp_order = nullptr;  // the solver leaves the order alone
  return true;
}

// The diagnostic dumps of an alignment: every block's stamps (NGICP_DEBUG_STAMPS), the last solver launch's stamps (_SOLVE, printed), when and
// where every block of the last pass ran (_SPAN), per-query search statistics of the last pass (_QSTATS), the groups' costs (_COSTS).
// debug_begin sizes and clears the buffers and sets the kernels' pointers, debug_end reads them back and writes the files.
struct DebugDumps {
  const char *stamp_path, *span_path, *qstat_path;  // null: not asked for
};
void* cleared(ngicp* h, DevBuf& b, size_t bytes) {
  b.ensure(bytes);
  HIP_TRY(hipMemsetAsync(b.p, 0, bytes, h->stream));
  return b.p;
}
void dump_to_file(const char* path, const void* dev, size_t bytes) {
  std::vector<unsigned char> host(bytes);
  HIP_TRY(hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost));
  if (FILE* f = std::fopen(path, "wb")) {
    std::fwrite(host.data(), 1, bytes, f);
    std::fclose(f);
  }
}
DebugDumps debug_begin(ngicp* h, LoopCtx& c) {
  const DebugDumps d{std::getenv("NGICP_DEBUG_STAMPS"), std::getenv("NGICP_DEBUG_SPAN"), std::getenv("NGICP_DEBUG_QSTATS")};  // diagnostic only
  if (d.stamp_path) c.pa.dbg_stamps = static_cast<unsigned long long*>(cleared(h, h->dbg, (size_t)(c.nblocks + 1) * 4 * kStampStride * sizeof(unsigned long long)));  // (k_gicp_head has one block more)
  if (std::getenv("NGICP_DEBUG_SOLVE")) c.sa.dbg_stamps = static_cast<unsigned long long*>(cleared(h, h->dbg_s, 8 * sizeof(unsigned long long)));
  if (d.span_path) c.pa.dbg_span = static_cast<unsigned long long*>(cleared(h, h->dbg_span, (size_t)c.nblocks * 4 * sizeof(unsigned long long)));
  if (d.qstat_path) c.pa.dbg_qstats = static_cast<int4*>(cleared(h, h->dbg_q, (size_t)c.pa.n_src * 2 * sizeof(int4)));
  return d;
}
void debug_end(ngicp* h, const LoopCtx& c, const DebugDumps& d) {
  if (d.stamp_path) dump_to_file(d.stamp_path, h->dbg.p, (size_t)(c.nblocks + 1) * 4 * kStampStride * sizeof(unsigned long long));
  if (c.sa.dbg_stamps) {
    unsigned long long ts[8];
    HIP_TRY(hipMemcpy(ts, h->dbg_s.p, sizeof(ts), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "k_lm_solve stamps (cycles since entry): loads issued %llu, reduced %llu, state in registers %llu, lm_advance %llu, accept path %llu, stored %llu; launch-order section (wave 1) %llu cycles\n",
                 ts[1] - ts[0], ts[2] - ts[0], ts[3] - ts[0], ts[4] - ts[0], ts[5] - ts[0], ts[6] - ts[0], ts[7]);
  }
  if (d.span_path) dump_to_file(d.span_path, h->dbg_span.p, (size_t)c.nblocks * 4 * sizeof(unsigned long long));
  if (const char* cost_path = std::getenv("NGICP_DEBUG_COSTS")) {  // diagnostic only: the groups' durations in the last pass (cycles >> 4), the launch order, the partial rows
    std::vector<int> hc((size_t)c.nblocks * 2);
    HIP_TRY(hipMemcpy(hc.data(), h->grp_cost.p, (size_t)c.nblocks * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hc.data() + c.nblocks, h->grp_order.p, (size_t)c.nblocks * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<double> hp((size_t)c.nblocks * kNumSlots);
    HIP_TRY(hipMemcpy(hp.data(), h->partials.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(cost_path, "wb")) {
      std::fwrite(hc.data(), sizeof(int), hc.size(), f);
      std::fwrite(hp.data(), sizeof(double), hp.size(), f);
      std::fclose(f);
    }
  }
  if (d.qstat_path) dump_to_file(d.qstat_path, h->dbg_q.p, (size_t)c.pa.n_src * 2 * sizeof(int4));
}

// ---- NGICP_PERSIST=1 (experiment, round 3): ONE launch for the whole alignment (k_gicp_persist): as many blocks as are resident
//      together, each keeping its groups pass after pass; the last block to finish a pass steps the optimiser and releases the next
//      one.  The idea: no second dispatch, no kernel boundaries - and with them no cold caches (a launch boundary drops every L2, and
//      ~9 of 10 L2 read requests of a pass go out to the fabric: profiles/r03_c3_pass_counters.json).  Measured (profiles/
//      r03_persistent_kernel.txt): bit-identical results; the groups run 4 % faster, but every hop of the grid-wide meeting (rows
//      written through, ticket, state, release word, view) is a ~1-2 us round trip to memory, as long as the launches they replace:
//      c3 50.7 us per iteration against 48.2, c5 76 against 58 (it has no 4-waves build).  So the default stays one launch per pass.
//      Launched cooperatively: the runtime guarantees that the grid is resident as a whole (the blocks wait for each other), and
//      one alignment per device at a time takes this route. ----
// true: the alignment is finished, al holds its final state.  false: the route was not taken (another alignment of this device is on it),
// or the kernel could not be launched or gave up - the state is back at the guess, and the alignment takes one launch per pass.
bool align_persistent(ngicp* h, const LoopCtx& c, Alignment& al, long max_passes) {
  const std::unique_lock<std::mutex> lock(persist_mutex(h->device), std::try_to_lock);
  if (!lock.owns_lock()) return false;
  int* const ctl = h->order_flag.as<int>();
  const int sel = h->order_sel;
  // {flag 0, ticket, gen, flag 1}: ticket and gen start at zero, and so does the flag of the buffer this alignment's solver will fill
  HIP_TRY(hipMemsetAsync(ctl + (sel == 0 ? 1 : 0), 0, 3 * sizeof(int), h->stream));
  HIP_TRY(hipMemsetAsync(h->gen_lines.p, 0, (size_t)kGenLines * kGenStride * sizeof(int), h->stream));
  PassArgs pa = c.pa;
  pa.fused = 1;
  pa.persist = 1;
  pa.max_passes = (int)max_passes;
  pa.sa = c.sa;
  pa.sa.persist = 1;
  pa.sa.grp_order = sel == 0 ? h->grp_order_alt.as<int>() : h->grp_order.as<int>();
  pa.sa.order_valid = sel == 0 ? ctl + 3 : ctl;
  pa.sa.pass_ticks = (h->profiling && max_passes <= kMaxTickPasses) ? h->pin_ticks : nullptr;
  const int grid = std::min(c.nblocks, h->persist_slots);
  void* kargs[] = {&pa};
  bool launched_ok = true;
  if (route::switches().persist_coop) {
    const hipError_t le = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(&k_gicp_persist<2, 3>), dim3((unsigned)grid), dim3(256), kargs, 0, h->stream);
    if (le != hipSuccess) {  // (e.g. the runtime finds the grid too large to be resident: one launch per pass then)
      (void)hipGetLastError();
      launched_ok = false;
    }
  } else {  // (A/B timing only: an ordinary launch relies on nothing else running on the device)
    hipLaunchKernelGGL((k_gicp_persist<2, 3>), dim3((unsigned)grid), dim3(256), 0, h->stream, pa);
  }
  bool ok = false;
  while (launched_ok) {
    const int prog = __atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE);
    if (prog & kProgressDone) {
      ok = true;
      break;
    }
    if ((++al.spins & 0x3fff) == 0) {
      if (hipStreamQuery(h->stream) == hipSuccess) {  // the kernel has left: done flag (then it is in memory by now), or its blocks gave up waiting
        ok = (__atomic_load_n(h->h_progress, __ATOMIC_ACQUIRE) & kProgressDone) != 0;
        break;
      }
      if (now_ms() - al.t_loop > 30000.0) throw ArgError{NGICP_ERR_HIP, "the registration loop did not finish within 30 s"};
    }
    if (h->host_wait) sched_yield(); else __builtin_ia32_pause();
  }
  if (ok) {
    al.st.hot = *h->pin_final;
    al.loop_ms = (float)((double)(al.st.hot.t_done - al.st.hot.t_first) * 1e-5);
    if (al.st.hot.passes >= 3 && c.nblocks <= kMaxOrderGroups) h->order_sel = sel ^ 1;  // the solver of the third pass left a fresh order in the other buffer
    return true;
  }
  // (never seen: the blocks' bounded wait ran out - e.g. the grid was not resident as a whole.  The state goes back to the guess and the
  // alignment takes one launch per pass.)
  std::fprintf(stderr, launched_ok ? "ngicp: the persistent registration kernel gave up waiting; falling back to one launch per pass\n"
                                   : "ngicp: the persistent registration kernel could not be launched; falling back to one launch per pass\n");
  h->persist = 0;
  HIP_TRY(hipMemsetAsync(h->order_flag.p, 0, 4 * sizeof(int), h->stream));
  HIP_TRY(hipMemcpyAsync(h->state.p, &h->pin_state[0], sizeof(LmState), hipMemcpyHostToDevice, h->stream));
  *h->h_progress = 0;
  return false;
}

void sum_tick_pass_times(ngicp* h, const LmHot& hot) {
  ngicp_stats& s = h->stats;
  // the persistent kernel's own stamps (100 MHz): a pass lasts from its release (the first: the alignment's first stamp) to the arrival
  // of its last block; the optimiser's step and the release that follows are not part of it
  const long timed = std::min<long>(hot.passes, kMaxTickPasses);
  int counted = 0;
  if (max_trace_rows(h->p) <= kMaxTickPasses) {  // (the LM bound, whatever the optimiser)
    for (long i = 0; i < timed; ++i) {
      const unsigned long long from = i == 0 ? hot.t_first : h->pin_ticks[2 * (i - 1) + 1], to = h->pin_ticks[2 * i];
      if (to > from) {
        s.pass_ms_total += (double)(to - from) * 1e-5;
        ++counted;
      }
    }
  }
  s.passes_timed = counted;
  if (std::getenv("NGICP_DEBUG_TICKS")) {  // diagnostic only: every pass and every step of the alignment, in microseconds
    std::fprintf(stderr, "persistent kernel, pass / step us:");
    for (long i = 0; i < timed; ++i) {
      const unsigned long long from = i == 0 ? hot.t_first : h->pin_ticks[2 * (i - 1) + 1];
      std::fprintf(stderr, " %.1f/%.1f", (double)(h->pin_ticks[2 * i] - from) * 1e-2, (double)(h->pin_ticks[2 * i + 1] - h->pin_ticks[2 * i]) * 1e-2);
    }
    std::fprintf(stderr, "\n");
  }
}

// ---- NGICP_HEAD=1: no solver launch at all (k_gicp_head): one launch per iteration, and one more whose head consumes the last pass ----
// its workspace: {done flag (64 B), subset tickets (128 B), subset rows of even / odd launches (2 x 8 KB)}, and the second state buffer
constexpr size_t kHeadCrowBytes = (size_t)kSolveRowSubsets * kNumSlots * sizeof(double);
void head_begin(ngicp* h) {
  h->state_alt.ensure(sizeof(LmState));
  h->head_ws.ensure(64 + 128 + 2 * kHeadCrowBytes);
  HIP_TRY(hipMemsetAsync(h->head_ws.p, 0, 64 + 128 + 2 * kHeadCrowBytes, h->stream));
}
// k_gicp_head: launch i reads state / subset rows / launch order [i & 1] and leaves the next ones in [(i + 1) & 1]
void launch_head(ngicp* h, const LoopCtx& c, long launched, hipEvent_t start, hipEvent_t stop) {
  unsigned char* const ws = h->head_ws.as<unsigned char>();
  int* const ctl = h->order_flag.as<int>();
  LmState* const state[2] = {h->state.as<LmState>(), h->state_alt.as<LmState>()};
  double* const crow[2] = {reinterpret_cast<double*>(ws + 192), reinterpret_cast<double*>(ws + 192 + kHeadCrowBytes)};
  int* const order[2] = {h->grp_order.as<int>(), h->grp_order_alt.as<int>()};
  int* const flag[2] = {ctl, ctl + 3};
  const int par = (int)(launched & 1);
  PassArgs pa = c.pa;
  pa.st = state[par];
  pa.crow_in = crow[par];
  pa.crow_out = crow[par ^ 1];
  pa.cluster_ticket = reinterpret_cast<int*>(ws + 64);
  pa.done_flag = reinterpret_cast<int*>(ws);
  pa.grp_order = order[par];
  pa.order_valid = flag[par];
  pa.sa = c.sa;
  pa.sa.st = state[par];
  pa.sa.st_out = state[par ^ 1];
  pa.sa.partials = crow[par];
  pa.sa.nrows = kSolveRowSubsets;
  pa.sa.grp_order = order[par ^ 1];
  pa.sa.order_valid = flag[par ^ 1];
  hipExtLaunchKernelGGL((k_gicp_head<2, 3>), dim3((unsigned)c.nblocks + 1), dim3(256), 0, h->stream, start, stop, 0, pa);
}

// NGICP_PERSIST_ONE (A/B only): the persistent kernel's code, one launch per pass
void launch_persist_one(ngicp* h, const LoopCtx& c, long launched, hipEvent_t start, hipEvent_t stop) {
  PassArgs pa = c.pa;
  pa.fused = 1;
  pa.persist = route::switches().persist_one;
  pa.first_pass = (int)launched;
  pa.max_passes = 1;
  pa.sa = c.sa;
  pa.sa.persist = 1;
  HIP_TRY(hipMemsetAsync(pa.ticket, 0, sizeof(int), h->stream));
  HIP_TRY(hipMemsetAsync(h->gen_lines.p, 0, (size_t)kGenLines * kGenStride * sizeof(int), h->stream));
  hipExtLaunchKernelGGL((k_gicp_persist<2, 3>), dim3((unsigned)std::min(c.nblocks, h->persist_slots)), dim3(256), 0, h->stream, start, stop, 0, pa);
}

// Refuse, prepare, choose the route (route::choose_route: the precedence is written down there), feed it.
void do_align(ngicp* h, const float guess[16], float* aligned, size_t out_stride) {
  refuse_route(h, route::Caller::Align, "ngicp_align");
  Alignment al;
  reset_results(h);
  LoopCtx c;
  prepare_loop(h, c);
  // the launch order the previous align ended with is still a good guess when the source index is the same one
  // (same batches; the costs come mostly from where the batches lie): the first pass then starts sorted as well
  // (the flag lives in a device word of its own: the solver sets it when an order is complete, the host only clears it when the
  // source index or the group count changed - it never has to read it back)
  if (!(h->order_src == h->src.dev.get() && h->order_groups == c.sa.nblocks)) HIP_TRY(hipMemsetAsync(h->order_flag.p, 0, 4 * sizeof(int), h->stream));  // (both flags)
  route::Facts f = route_facts(h, route::Caller::Align, c.nblocks);
  f.xcd_installed = install_xcd_order(h, c);
  set_pass_mode(h, c.pa);
  allow_k4_only_passes(h, c, f);
  if (const char* dbg = std::getenv("NGICP_DEBUG_MODE")) c.pa.mode |= (std::atoi(dbg) & (8 | 16));  // timing experiments only
  begin_alignment(h, al, guess, c.sa, c.pa.t_first);
  const DebugDumps dbg = debug_begin(h, c);
  f.dump_stamps = dbg.stamp_path != nullptr;
  f.dump_span = dbg.span_path != nullptr;
  f.dump_qstats = dbg.qstat_path != nullptr;
  f.dump_solve = c.sa.dbg_stamps != nullptr;
  const route::Choice pick = route::choose_route(route::switches(), h->sw, f);
  const long max_p = f.max_passes;
  const bool persist_done = pick.route == route::Route::Persist && align_persistent(h, c, al, max_p);
  switch (persist_done ? route::Route::Persist : pick.fallback) {
    case route::Route::Persist:  // (one launch has run the whole alignment)
      break;
    case route::Route::Head:
      head_begin(h);
      feed_alignment(h, al, max_p + 1, [&](long i, hipEvent_t start, hipEvent_t stop) { launch_head(h, c, i, start, stop); });
      // (k_gicp_head: the head of launch `passes` ended the alignment and left the final state in the buffer it does not read; the handle's
      // other entry points look for it in h->state)
      if ((al.st.hot.passes + 1) & 1) HIP_TRY(hipMemcpyAsync(h->state.p, h->state_alt.p, sizeof(LmState), hipMemcpyDeviceToDevice, h->stream));
      break;
    case route::Route::PersistOne:
      feed_alignment(h, al, max_p, [&](long i, hipEvent_t start, hipEvent_t stop) { launch_persist_one(h, c, i, start, stop); });
      break;
    case route::Route::Fused:
      // NGICP_FUSED=1: one dispatch per iteration - the last block of the pass reduces and advances the optimiser (PassArgs::fused).
      // Measured on MI355X (round 3, profiles/r03_fused_solver.txt): bit-identical results, but no faster than the separate launch (c3
      // 46.3 vs 45.4 us per iteration, c5 70 vs 56): the write-through rows come back from memory, not from L2, through ONE CU
      // (8.7 k cycles for 222 KB against 5.5 k in k_lm_solve), plus the acquire (~1.7 us) - so the default stays two launches.
      c.pa.fused = 1;
      c.pa.sa = c.sa;
      HIP_TRY(hipMemsetAsync(c.pa.ticket, 0, sizeof(int), h->stream));
      [[fallthrough]];
    case route::Route::Default:
    case route::Route::Staged:
    case route::Route::Queue: {
      // (diagnostic only) NGICP_DEBUG_SOLVE=N, N > 1: the stamps of the solver launch behind pass N - one that makes a trial, where the
      // last launch of an alignment only ends it; 1: of the last working launch
      const long stamp_launch = route::switches().debug_solve_launch;
      feed_alignment(h, al, max_p, [&](long i, hipEvent_t start, hipEvent_t stop) {
        launch_pass(h, c.pa, pick.variant, c.nblocks, h->stream, start, stop);
        if (!route::row(pick.fallback).own_solver) return;
        SolveArgs sa = c.sa;
        if (stamp_launch > 1 && i + 1 != stamp_launch) sa.dbg_stamps = nullptr;
        hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, sa);
      });
      break;
    }
  }
  HIP_TRY(hipGetLastError());
  debug_end(h, c, dbg);
  end_alignment(h, al, aligned, out_stride, !persist_done);
  ngicp_stats& s = h->stats;
  h->order_src = h->src.dev.get();  // (what the order flag on the device, if set, refers to)
  h->order_groups = c.sa.nblocks;
  s.staged_fraction = al.st.hot.search_passes > 0 ? al.st.hot.staged_total / ((double)al.st.hot.search_passes * (double)h->src.dev->n) : 0.0;
  if (al.st.hot.search_passes > 1) h->prev_staged_fraction = s.staged_fraction;  // (the first pass lists for every batch or for none: it says nothing)
  if (persist_done && h->profiling) sum_tick_pass_times(h, al.st.hot);
}

struct VoxelCtx {
  VoxelPassArgs pa;
  SolveArgs sa;
  int nblocks;
};

// (neighbourhood, robust) -> the instantiation: f(integral_constant<int, K>, bool_constant<ROBUST>) for the K of DIRECT1 / 7 / 27
template <class F>
void with_voxel_variant(int nbr, bool robust, F&& f) {
  auto with_k = [&](auto k) { robust ? f(k, std::true_type{}) : f(k, std::false_type{}); };
  switch (nbr) {
    case NGICP_VOX_DIRECT1: with_k(std::integral_constant<int, 1>{}); break;
    case NGICP_VOX_DIRECT7: with_k(std::integral_constant<int, 7>{}); break;
    case NGICP_VOX_DIRECT27: with_k(std::integral_constant<int, 27>{}); break;
    default: throw ArgError{NGICP_ERR_STATE, "voxelized GICP: unknown neighbourhood"};
  }
}

// the pass of the neighbourhood in c.pa.nbr: k_vgicp_pass for DIRECT1, k_vgicp_pass_n<K> for DIRECT7 / DIRECT27; the same grid
void launch_voxel_pass(ngicp* h, const VoxelCtx& c, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  const dim3 grid((unsigned)c.nblocks), block(kVoxBlock);
  with_voxel_variant(c.pa.nbr, c.pa.robust_kind != NGICP_ROBUST_NONE, [&](auto k, auto robust) {
    constexpr int K = decltype(k)::value;
    constexpr bool R = decltype(robust)::value;
    if constexpr (K == 1) hipExtLaunchKernelGGL(k_vgicp_pass<R>, grid, block, 0, h->stream, start, stop, 0, c.pa);
    else hipExtLaunchKernelGGL((k_vgicp_pass_n<K, R>), grid, block, 0, h->stream, start, stop, 0, c.pa);
  });
}

// the fields of a voxelized pass that do not depend on the alignment (or the lane): the source, the map, the neighbourhood
void fill_voxel_shared(ngicp* h, VoxelPassArgs& a, const VoxelMapView& m) {
  DeviceCloud& S = *h->src.dev;
  a.src = S.pts();
  a.cov_src = covs_for(h, h->src_covs, h->src.dev);
  a.n_src = (int)S.n;
  a.table = m.table;
  a.mask = m.mask;
  a.rec = m.rec;
  a.n_vox = (int)m.n_vox;
  a.inv_res = 1.0f / (float)h->voxel_res;
  a.nbr = h->voxel_nbr;
  a.slot_stride = (int)S.n;
  a.mode = 3;
  a.t_first = nullptr;
  fill_robust(h, a.robust_kind, a.robust_c, a.robust_c2);
}

// prepare_loop readies the slots, the covariances, the state, the trace and the solver's arguments exactly as for the exact path; the
// voxelized pass then brings its own grid (256 source points per block), its own rows and correspondence buffers.  The launch order of
// the exact pass's groups (grp_order, its flag) is neither read nor written.
void prepare_voxel_loop(ngicp* h, VoxelCtx& v) {
  LoopCtx c;
  prepare_loop(h, c, true, !rolling_active(h));
  const VoxelMapView vm = ensure_voxel_map(h);
  DeviceCloud& S = *h->src.dev;
  const size_t n = S.n;
  const int nblocks = std::max(1, (int)((n + kVoxBlock - 1) / kVoxBlock));
  h->partials.ensure((size_t)kNumSlots * nblocks * sizeof(double));
  // slot-major state of the neighbourhood in use: corr[2][K][n] ints, and for K > 1 mahal[2][K][n][6] doubles (2 * K * 52 bytes a point)
  const size_t K = (size_t)h->voxel_nbr;
  for (int i = 0; i < 2; ++i) {
    h->vox_corr[i].ensure(K * n * sizeof(int));
    if (K > 1) h->vox_mahal[i].ensure(K * n * 6 * sizeof(double));
  }
  VoxelPassArgs& a = v.pa;
  fill_voxel_shared(h, a, vm);
  for (int i = 0; i < 2; ++i) {
    a.corr[i] = h->vox_corr[i].as<int>();
    a.mahal[i] = K > 1 ? h->vox_mahal[i].as<double>() : h->mahal[i].as<double>();
  }
  a.st = h->state.as<LmState>();
  a.partials = h->partials.as<double>();
  v.sa = c.sa;
  v.sa.partials = a.partials;
  v.sa.nblocks = nblocks;
  v.sa.grp_order = nullptr;  // (the solver sorts nothing)
  v.sa.grp_cost = nullptr;
  v.sa.order_valid = nullptr;
  v.nblocks = nblocks;
}

// do_align for a voxelized target: the same loop - state upload, (pass, solve) pairs fed NGICP_CHUNK ahead of the solver's published
// progress, the final state read from pinned memory - with k_vgicp_pass in k_gicp_pass's place.  None of the exact path's kernel-variant
// switches applies.
void do_align_voxel(ngicp* h, const float guess[16], float* aligned, size_t out_stride) {
  Alignment al;
  reset_results(h);
  VoxelCtx c;
  prepare_voxel_loop(h, c);
  c.pa.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  begin_alignment(h, al, guess, c.sa, c.pa.t_first);
  feed_alignment(h, al, max_passes(h->p), [&](long, hipEvent_t start, hipEvent_t stop) {
    launch_voxel_pass(h, c, start, stop);
    hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, c.sa);
  });
  HIP_TRY(hipGetLastError());
  end_alignment(h, al, aligned, out_stride);  // (mean_candidates: this mode tests no target point, it counts the hash-table slots looked at)
  h->stats.staged_fraction = 0.0;
}

// One pass with mode bits `pass_mode`, then k_lm_solve in mode `solve_mode`, on the handle's state: the exact pass or the voxelized one,
// whichever the handle is set to (ngicp_linearize, ngicp_compute_error).
struct HookCtx {
  bool vox;
  LoopCtx c;
  VoxelCtx vc;
  route::Variant variant;  // the exact pass's kernel
};
void prepare_hook(ngicp* h, HookCtx& k) {
  k.vox = h->voxel_res > 0.0;
  if (k.vox) {
    prepare_voxel_loop(h, k.vc);
    return;
  }
  refuse_route(h, route::Caller::Hook, "linearize / compute_error");
  prepare_loop(h, k.c);
  k.variant = pass_variant(h, route::Caller::Hook, k.c.nblocks);
}
void launch_hook(ngicp* h, HookCtx& k, int pass_mode, int solve_mode) {
  if (k.vox) {
    k.vc.pa.mode = pass_mode;
    launch_voxel_pass(h, k.vc);
  } else {
    k.c.pa.mode = pass_mode;
    launch_pass(h, k.c.pa, k.variant, k.c.nblocks, h->stream);
  }
  SolveArgs sa = k.vox ? k.vc.sa : k.c.sa;
  sa.mode = solve_mode;
  hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(kSolveThreads), 0, h->stream, sa);
}

// ------------------------------------------------------------------------------------------
// Batched registration: several initial guesses on one source / target pair
// ------------------------------------------------------------------------------------------
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void ensure_batch_pinned(ngicp* h) {
  BatchWs& w = h->batch;
  if (!w.pin_recs) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w.pin_recs), (size_t)kBatchMaxLanes * (sizeof(LmState) + sizeof(PassArgs) + sizeof(SolveArgs)), hipHostMallocDefault));
  if (!w.pin_progress) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w.pin_progress), (size_t)kBatchMaxLanes * BatchWs::kProgressStride * sizeof(int), hipHostMallocDefault));
  if (!w.pin_final) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w.pin_final), (size_t)kBatchMaxLanes * sizeof(LmHot), hipHostMallocDefault));
}

// The feeding loop of a batch, shared by ngicp_align_batch and ngicp_voxel_align_batch: the lane records are on the device, every
// lane's progress word in pinned memory is 0; launch_pass_batch(bl, n_live) enqueues one pass launch that serves the n_live lanes listed
// in bl.lane, and one k_lm_solve_batch launch behind it steps their optimisers.  result[g]: lane g's final state image.
template <class LaunchPass>
void feed_batch(ngicp* h, int B, BatchLaunch& bl, long max_passes, std::vector<LmHot>& result, LaunchPass&& launch_pass_batch) {
  BatchWs& w = h->batch;
  // The feeding discipline of do_align: (pass, solve) pairs kept `depth` ahead of the slowest live lane's progress word.  A lane that
  // reports done leaves the list; its blocks in the launches already enqueued return at their head.
  const int depth = h->sw.chunk;
  const double t_loop = now_ms();
  unsigned long spins = 0;
  bool idle_seen = false;
  // Every so many polls the stream is asked for its status: an asynchronous error comes out as its HIP error, not as the timeout.
  // true: the stream has nothing left to run.
  auto look_at_stream = [&]() -> bool {
    const hipError_t q = hipStreamQuery(h->stream);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
    } else if (q != hipSuccess) {
      throw HipError{q, "hipStreamQuery(h->stream)", __FILE__, __LINE__};
    }
    if (now_ms() - t_loop > 30000.0) throw ArgError{NGICP_ERR_HIP, "the batched registration loop did not finish within 30 s"};
    return q == hipSuccess;
  };
  auto relax = [&]() {
    // (idle at the last look: every launch enqueued had run, so the words the caller has just read again were final)
    if (idle_seen) throw ArgError{NGICP_ERR_HIP, "the batched registration loop: the stream is idle but a lane has not reported"};
    if ((++spins & (h->host_wait ? 0xff : 0xfff)) == 0 && look_at_stream()) {
      idle_seen = true;
      return;
    }
    if (h->host_wait) sched_yield(); else __builtin_ia32_pause();
  };
  long launched = 0;
  int n_live = B;
  std::vector<int> live((size_t)B);
  for (int g = 0; g < B; ++g) live[(size_t)g] = g;
  for (;;) {
    long min_prog = std::numeric_limits<long>::max();
    int keep_n = 0;
    for (int i = 0; i < n_live; ++i) {
      const int g = live[(size_t)i];
      const int prog = __atomic_load_n(w.pin_progress + (size_t)g * BatchWs::kProgressStride, __ATOMIC_ACQUIRE);
      if (prog & kProgressDone) {
        result[(size_t)g] = w.pin_final[g];  // (stored before the flag: lm_solve_body)
        continue;
      }
      live[(size_t)keep_n++] = g;
      min_prog = std::min(min_prog, (long)(prog & kProgressMask));
    }
    n_live = keep_n;
    if (n_live == 0) break;
    if (launched >= max_passes || launched - min_prog >= depth) {  // enough in flight (or nothing left to launch: the last possible pass sets done)
      relax();
      continue;
    }
    idle_seen = false;
    for (int i = 0; i < n_live; ++i) bl.lane[i] = live[(size_t)i];
    launch_pass_batch(bl, n_live);
    hipLaunchKernelGGL(k_lm_solve_batch, dim3((unsigned)n_live), dim3(kSolveThreads), 0, h->stream, bl);
    ++launched;
  }
}

// every lane's final state into the caller's arrays, and the description of the traces ngicp_batch_get_lm_trace serves
void return_batch_results(ngicp* h, const std::vector<LmHot>& result, size_t trace_stride, float* T_out, int* converged, int* nr_iterations, double* hessians) {
  BatchWs& w = h->batch;
  for (size_t g = 0; g < result.size(); ++g) {
    store_result(result[g], T_out + g * 16, converged ? converged + g : nullptr, nr_iterations ? nr_iterations + g : nullptr, hessians ? hessians + g * 36 : nullptr);
    w.trace_rows.push_back((size_t)result[g].n_trace);
  }
  w.lanes = (int)result.size();
  w.trace_stride = trace_stride;
}

// ---- the front end ngicp_align_batch and ngicp_voxel_align_batch share: the lane records and what is done with them ----
// Where a call's records lie - [B] LmState images, then [B] pass records, then [B] SolveArgs - in the pinned block and on the device, and the
// strides of the per-lane rows and traces.
struct BatchRecs {
  int B;
  size_t off_pass, off_solve, bytes, part_stride, trace_stride;
  LmState* st_host;
  unsigned char* pass_host;
  SolveArgs* sa_host;
  unsigned char* dev;
};

// Forgets the previous call's traces and sizes what both entries use: the records (pass records of pass_size bytes), nblocks rows per lane,
// the traces.  (Every buffer is sized before the first launch: growing one frees it, and freeing waits for the device.)
BatchRecs batch_begin(ngicp* h, int B, size_t pass_size, int nblocks) {
  BatchWs& w = h->batch;
  BatchRecs r;
  r.B = B;
  r.off_pass = (size_t)B * sizeof(LmState);
  r.off_solve = r.off_pass + round_up((size_t)B * pass_size, 16);
  r.bytes = r.off_solve + (size_t)B * sizeof(SolveArgs);
  r.part_stride = (size_t)nblocks * kNumSlots * sizeof(double);
  r.trace_stride = (size_t)max_trace_rows(h->p) * kTraceCols;
  w.lanes = 0;  // (the traces of the previous call go with the buffers)
  w.trace_rows.clear();
  ensure_batch_pinned(h);
  w.recs.ensure(r.bytes);
  w.partials.ensure((size_t)B * r.part_stride);
  w.trace.ensure((size_t)B * r.trace_stride * sizeof(double));
  r.st_host = reinterpret_cast<LmState*>(w.pin_recs);
  r.pass_host = w.pin_recs + r.off_pass;
  r.sa_host = reinterpret_cast<SolveArgs*>(w.pin_recs + r.off_solve);
  r.dev = w.recs.as<unsigned char>();
  return r;
}

// Lane g's state image from its guess, its progress word zeroed, and its solver record: `shared` with the lane's state, rows, trace and
// pinned words.  The caller completes the record and stores it with the lane's pass record.
SolveArgs batch_lane(ngicp* h, const BatchRecs& r, int g, const float* guesses, const SolveArgs& shared) {
  BatchWs& w = h->batch;
  init_state_from_pose(r.st_host[g], pose_from_colmajor(guesses + (size_t)g * 16));
  if (h->p.max_iter <= 0) r.st_host[g].hot.done = 1;
  SolveArgs sa = shared;
  sa.st = reinterpret_cast<LmState*>(r.dev) + g;
  sa.partials = reinterpret_cast<double*>(w.partials.as<unsigned char>() + (size_t)g * r.part_stride);
  sa.trace = w.trace.as<double>() + (size_t)g * r.trace_stride;
  sa.progress_host = w.pin_progress + (size_t)g * BatchWs::kProgressStride;
  sa.final_host = w.pin_final + g;
  sa.t_first = nullptr;
  *sa.progress_host = 0;
  return sa;
}

// The records are complete: one upload, the feeding loop with the entry's pass launch, every lane's results into the caller's arrays.
template <class LaunchPass>
void run_batch(ngicp* h, const BatchRecs& r, float* T_out, int* converged, int* nr_iterations, double* hessians, LaunchPass&& launch_pass_batch) {
  std::vector<LmHot> result((size_t)r.B);
  if (h->p.max_iter <= 0) {
    for (int g = 0; g < r.B; ++g) result[(size_t)g] = r.st_host[g].hot;  // every lane returns its guess, as ngicp_align does; nothing is launched
  } else {
    HIP_TRY(hipMemcpyAsync(r.dev, h->batch.pin_recs, r.bytes, hipMemcpyHostToDevice, h->stream));  // ONE upload
    BatchLaunch bl;
    bl.pass = r.dev + r.off_pass;
    bl.solve = reinterpret_cast<const SolveArgs*>(r.dev + r.off_solve);
    for (int i = 0; i < kBatchMaxLanes; ++i) bl.lane[i] = 0;
    feed_batch(h, r.B, bl, max_passes(h->p), result, launch_pass_batch);
    HIP_TRY(hipGetLastError());
  }
  return_batch_results(h, result, r.trace_stride, T_out, converged, nr_iterations, hessians);
}

// The batch always takes the default route: walks in global memory (k_gicp_pass_batch), a solver launch of its own (k_lm_solve_batch).
// NGICP_PERSIST, NGICP_HEAD, NGICP_FUSED, NGICP_QUEUE, NGICP_PASS_IMPL and NGICP_ORDER do not apply to it.
void do_align_batch(ngicp* h, int B, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* hessians) {
  BatchWs& w = h->batch;
  // (slots, lazy covariances, the shared fields - and none of the handle's single-alignment buffers: what the getters of the last
  // ngicp_align read is neither resized nor written)
  LoopCtx c;
  prepare_loop(h, c, false);
  set_pass_mode(h, c.pa);  // (the decision an align on this handle would take now: do_align)

  const size_t n = h->src.dev->n;
  const int nblocks = c.nblocks, n_batches = c.pa.n_batches;
  const size_t tpt_stride = round_up(n * sizeof(float4), 256), mahal_stride = round_up(n * 6 * sizeof(double), 256);
  const size_t ord_stride = round_up((size_t)nblocks * sizeof(int), 256), far_stride = round_up((size_t)n_batches + 16, 256);
  // (a call that fails half way - an allocation, say - must not leave a description of launch orders that a replaced buffer no longer holds)
  const bool order_described = w.order_src == h->src.dev.get() && w.order_groups == nblocks && w.order_lanes >= B;
  const int lanes_before = w.order_lanes;
  w.order_src = nullptr;
  w.order_lanes = 0;
  const BatchRecs r = batch_begin(h, B, sizeof(PassArgs), nblocks);
  w.tpt.ensure((size_t)B * 2 * tpt_stride);
  w.mahal.ensure((size_t)B * 2 * mahal_stride);
  bool order_kept = order_described;
  if (w.order.ensure_grew((size_t)B * ord_stride)) order_kept = false;
  w.cost.ensure((size_t)B * ord_stride);
  if (w.flags.ensure_grew((size_t)kBatchMaxLanes * 4 * sizeof(int))) order_kept = false;
  if (w.far.ensure_grew((size_t)B * far_stride)) HIP_TRY(hipMemsetAsync(w.far.p, 0, w.far.cap, h->stream));
  // a lane's launch order of the previous call is still a good guess when the source index is the same one (do_align)
  if (!order_kept) HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)kBatchMaxLanes * 4 * sizeof(int), h->stream));

  PassArgs* const pa_host = reinterpret_cast<PassArgs*>(r.pass_host);
  for (int g = 0; g < B; ++g) {
    SolveArgs sa = batch_lane(h, r, g, guesses, c.sa);
    PassArgs pa = c.pa;
    pa.st = sa.st;
    for (int i = 0; i < 2; ++i) {
      pa.tpt[i] = reinterpret_cast<float4*>(w.tpt.as<unsigned char>() + ((size_t)g * 2 + i) * tpt_stride);
      pa.mahal[i] = reinterpret_cast<double*>(w.mahal.as<unsigned char>() + ((size_t)g * 2 + i) * mahal_stride);
    }
    pa.partials = const_cast<double*>(sa.partials);  // (the lane's own rows)
    pa.grp_order = reinterpret_cast<int*>(w.order.as<unsigned char>() + (size_t)g * ord_stride);
    pa.grp_cost = reinterpret_cast<int*>(w.cost.as<unsigned char>() + (size_t)g * ord_stride);
    pa.batch_far = w.far.as<unsigned char>() + (size_t)g * far_stride;
    pa.order_valid = w.flags.as<int>() + (size_t)g * 4;
    pa.ticket = w.flags.as<int>() + (size_t)g * 4 + 1;
    pa.t_first = nullptr;
    sa.grp_order = const_cast<int*>(pa.grp_order);
    sa.grp_cost = pa.grp_cost;
    sa.order_valid = const_cast<int*>(pa.order_valid);
    pa.sa = sa;
    pa_host[g] = pa;
    r.sa_host[g] = sa;
  }
  run_batch(h, r, T_out, converged, nr_iterations, hessians, [&](const BatchLaunch& l, int n_live) {
    const bool four = (long)nblocks * n_live > 2L * h->pass_slots;  // route::choose_route's rule on the whole grid
    if (four)
      hipLaunchKernelGGL((k_gicp_pass_batch<2, 4>), dim3((unsigned)nblocks, (unsigned)n_live), dim3(256), 0, h->stream, l);
    else
      hipLaunchKernelGGL((k_gicp_pass_batch<2, 3>), dim3((unsigned)nblocks, (unsigned)n_live), dim3(256), 0, h->stream, l);
  });
  w.order_src = h->src.dev.get();
  w.order_groups = nblocks;
  w.order_lanes = std::max(order_kept ? lanes_before : 0, B);
}

// ngicp_voxel_align_batch: do_align_batch's protocol - the lane records in one pinned block and one upload, a progress
// word and a final image per lane in pinned memory, the live lanes in the kernel arguments, feed_batch - with k_vgicp_pass_batch<K> in
// k_gicp_pass_batch's place and the solver's records as prepare_voxel_loop sets them (no launch order).  Every per-lane buffer is the
// batch's own: vox_corr / vox_mahal / mahal / state / partials / trace of the handle, which the getters of the last ngicp_align read,
// are neither resized nor written.  None of the exact path's kernel-variant switches applies.
void do_align_voxel_batch(ngicp* h, int B, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* hessians) {
  static_assert(sizeof(VoxelPassArgs) <= sizeof(PassArgs), "the pinned record block is sized for PassArgs records");
  BatchWs& w = h->batch;
  LoopCtx c;
  prepare_loop(h, c, false, !rolling_active(h));   // (slots, lazy covariances, the solver's configuration)
  const VoxelMapView vm = ensure_voxel_map(h);  // (at most one build, whatever the number of lanes)
  const size_t n = h->src.dev->n, K = (size_t)h->voxel_nbr;
  const int nblocks = std::max(1, (int)((n + kVoxBlock - 1) / kVoxBlock));
  const size_t corr_stride = round_up(K * n * sizeof(int), 256), mahal_stride = round_up(K * n * 6 * sizeof(double), 256);
  const BatchRecs r = batch_begin(h, B, sizeof(VoxelPassArgs), nblocks);
  w.vox_corr.ensure((size_t)B * 2 * corr_stride);
  w.vox_mahal.ensure((size_t)B * 2 * mahal_stride);
  VoxelPassArgs shared;
  fill_voxel_shared(h, shared, vm);
  shared.mode = (h->p.optimizer == NGICP_OPT_GAUSS_NEWTON) ? 2 : 3;
  SolveArgs solve = c.sa;
  solve.nblocks = nblocks;
  solve.grp_order = nullptr;  // (the solver sorts nothing: prepare_voxel_loop)
  solve.grp_cost = nullptr;
  solve.order_valid = nullptr;
  VoxelPassArgs* const pa_host = reinterpret_cast<VoxelPassArgs*>(r.pass_host);
  for (int g = 0; g < B; ++g) {
    const SolveArgs sa = batch_lane(h, r, g, guesses, solve);
    VoxelPassArgs pa = shared;
    pa.st = sa.st;
    for (int i = 0; i < 2; ++i) {
      pa.corr[i] = reinterpret_cast<int*>(w.vox_corr.as<unsigned char>() + ((size_t)g * 2 + i) * corr_stride);
      pa.mahal[i] = reinterpret_cast<double*>(w.vox_mahal.as<unsigned char>() + ((size_t)g * 2 + i) * mahal_stride);
    }
    pa.partials = const_cast<double*>(sa.partials);  // (the lane's own rows)
    pa_host[g] = pa;
    r.sa_host[g] = sa;
  }
  run_batch(h, r, T_out, converged, nr_iterations, hessians, [&](const BatchLaunch& l, int n_live) {
    const dim3 grid((unsigned)nblocks, (unsigned)n_live), block(kVoxBlock);
    // (no robust build: the entry refuses the kernel)
    with_voxel_variant((int)K, false, [&](auto k, auto) { hipLaunchKernelGGL(k_vgicp_pass_batch<decltype(k)::value>, grid, block, 0, h->stream, l); });
  });
}

}  // namespace
