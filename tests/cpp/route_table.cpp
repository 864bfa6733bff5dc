// ngicp_route.h against the decision code it replaced.  The legacy_* functions are that code (do_align's conditions, launch_pass's ladder,
// robust_unsupported_switch, refuse_*_under_switch, honour_lin_unneeded with its guard, prepare_hook's check) with the function-local
// statics and the handle's members turned into fields of Old; the kernel launches are turned into the record of what would be launched.
// Over the whole cross product of switches and facts, route::choose_route, route::honours_lin_unneeded and route::refusal must agree with
// it - except that a robust kernel under NGICP_PERSIST_ONE is now refused.  Then the two readers' parsing and clamps, fed by a fake lookup.
// Needs no library: g++ -std=c++17 -Wall -Werror tests/cpp/route_table.cpp
#include <cstdio>
#include <cstring>
#include <string>

#include "../../direct_lidar_odometry_amd/csrc/ngicp_route.h"

namespace {

struct Old {
  // the process-wide statics
  int pass_impl, queue_env, force_wps;
  bool fused_env, xcd_order, persist_one;
  // struct ngicp's members
  int persist, head, full_last_pass, robust_kind, max_iter, pass_slots, persist_slots;
  bool prior_set;
  // the alignment
  int nblocks;
  long max_p;
  bool stamp_path, span_path, qstat_path, solve_stamps;
};
struct Launch {  // which kernel a launch_pass call launches
  route::Family family;
  int waves;
  bool fused, robust;
};
struct PassArgsOld {
  int fused, mode, robust_kind;
  bool dbg_stamps, dbg_span, dbg_qstats;
};

const char* legacy_robust_unsupported_switch(const Old& h) {
  if (h.pass_impl == 1) return "NGICP_PASS_IMPL=1";
  if (h.fused_env) return "NGICP_FUSED";
  if (h.queue_env != 0) return "NGICP_QUEUE";
  if (h.persist) return "NGICP_PERSIST";
  if (h.head) return "NGICP_HEAD";
  return nullptr;
}
std::string legacy_refuse_robust_under_switch(const Old& h, const char* entry) {
  if (h.robust_kind == NGICP_ROBUST_NONE) return {};
  if (const char* sw = legacy_robust_unsupported_switch(h))
    return std::string(entry) + ": the robust kernel has no instantiation of the pass variant " + sw + " selects (unset it, or ngicp_set_robust_kernel(h, NGICP_ROBUST_NONE, 0))";
  return {};
}
std::string legacy_refuse_prior_under_switch(const Old& h, const char* entry) {
  if (h.prior_set && h.head)
    return std::string(entry) + ": the pose prior is not applied by the route NGICP_HEAD selects (unset it, or ngicp_set_pose_prior(h, NULL, NULL))";
  return {};
}
bool legacy_honour_lin_unneeded(const Old& h) {
  if (h.full_last_pass || h.pass_impl != 0 || h.queue_env) return false;
  return true;
}
Launch legacy_launch_pass(const Old& h, const PassArgsOld& a, int nblocks) {
  const int force = h.force_wps;
  const int impl = h.pass_impl;
  const bool four = force ? force == 4 : nblocks > 2 * h.pass_slots;
  if (impl == 1) {
    if (force ? force == 4 : true) return {route::Family::Staged, 4, false, false};
    return {route::Family::Staged, 3, false, false};
  }
  if (h.queue_env && !a.fused && !(a.mode & 4) && !a.dbg_stamps && !a.dbg_span && !a.dbg_qstats) return {route::Family::Queue, four ? 4 : 3, false, false};
  if (a.fused) return {route::Family::Walks, four ? 4 : 3, true, false};
  if (a.robust_kind != NGICP_ROBUST_NONE) return {route::Family::Walks, four ? 4 : 3, false, true};
  return {route::Family::Walks, four ? 4 : 3, false, false};
}

struct Outcome {
  route::Route route, fallback;
  bool has_launch;  // the fallback is a launch-per-pass route: `launch` is its kernel
  Launch launch;
  bool lin;
  std::string refusal;
};

route::Route route_of(const Launch& l) {
  if (l.family == route::Family::Staged) return route::Route::Staged;
  if (l.family == route::Family::Queue) return route::Route::Queue;
  return l.fused ? route::Route::Fused : route::Route::Default;
}

Outcome legacy_do_align(const Old& h) {
  Outcome o{};
  o.refusal = legacy_refuse_robust_under_switch(h, "ngicp_align");
  if (o.refusal.empty()) o.refusal = legacy_refuse_prior_under_switch(h, "ngicp_align");
  PassArgsOld pa{0, 3, h.robust_kind, h.stamp_path, h.span_path, h.qstat_path};
  const bool xcd_order = h.xcd_order;
  if (!h.persist && !h.head && !h.persist_one) o.lin = legacy_honour_lin_unneeded(h);
  if (o.lin) pa.mode |= 64;
  if (h.fused_env && h.pass_impl == 0) pa.fused = 1;
  const long max_p = h.max_p;
  const bool plain = h.max_iter > 0 && h.pass_impl == 0 && !pa.fused && !xcd_order && !h.span_path && !h.qstat_path && !h.solve_stamps;
  const bool want_persist = h.persist && plain && h.persist_slots > 0 && !h.stamp_path && max_p + 1 <= route::kMaxPersistPasses;
  const bool persist_done = false;  // (the fallback is what runs when align_persistent declines)
  const bool head_mode = h.head && plain && !persist_done && h.nblocks <= 2 * h.pass_slots;
  if (head_mode) {
    o.fallback = route::Route::Head;
  } else if (h.persist_one && h.persist_slots > 0 && max_p + 1 <= route::kMaxPersistPasses) {
    o.fallback = route::Route::PersistOne;
  } else {
    o.has_launch = true;
    o.launch = legacy_launch_pass(h, pa, h.nblocks);
    o.fallback = route_of(o.launch);
  }
  o.route = want_persist ? route::Route::Persist : o.fallback;
  return o;
}
Outcome legacy_hook(const Old& h, int pass_mode) {
  Outcome o{};
  if (h.robust_kind != NGICP_ROBUST_NONE && h.pass_impl == 1)
    o.refusal = "linearize / compute_error: the robust kernel has no instantiation of the pass variant NGICP_PASS_IMPL=1 selects";
  const PassArgsOld pa{0, pass_mode, h.robust_kind, false, false, false};
  o.has_launch = true;
  o.launch = legacy_launch_pass(h, pa, h.nblocks);
  o.route = o.fallback = route_of(o.launch);
  return o;
}
Outcome legacy_sharded(const Old& h) {  // ngicp_sharded_begin's mode, ngicp_sharded_pass's launch (robust and prior are refused at the entry)
  Outcome o{};
  o.lin = legacy_honour_lin_unneeded(h);
  const PassArgsOld pa{0, 3 | (o.lin ? 64 : 0), h.robust_kind, false, false, false};
  o.has_launch = true;
  o.launch = legacy_launch_pass(h, pa, h.nblocks);
  o.route = o.fallback = route_of(o.launch);
  return o;
}

long g_cells = 0, g_new_refusals = 0, g_bad = 0;

void compare(const Old& h, route::Caller caller, const Outcome& want, const route::ProcessSwitches& p, const route::HandleSwitches& w, const route::Facts& f, const char* entry) {
  ++g_cells;
  const route::Choice got = route::choose_route(p, w, f);
  const bool lin = route::honours_lin_unneeded(p, w, f);
  const std::string why = route::refusal(p, w, f, entry);
  bool ok = got.route == want.route && got.fallback == want.fallback && lin == want.lin;
  if (want.has_launch)
    ok = ok && got.variant.family == want.launch.family && got.variant.waves == want.launch.waves && got.variant.fused == want.launch.fused && got.variant.robust == want.launch.robust;
  if (caller == route::Caller::Align && h.robust_kind != NGICP_ROBUST_NONE && h.persist_one && want.refusal.empty()) {
    ++g_new_refusals;  // the one listed exception: k_gicp_persist has no robust instantiation either
    ok = ok && why == "ngicp_align: the robust kernel has no instantiation of the pass variant NGICP_PERSIST_ONE selects (unset it, or ngicp_set_robust_kernel(h, NGICP_ROBUST_NONE, 0))";
  } else {
    ok = ok && why == want.refusal;
  }
  if (!ok && ++g_bad <= 10)
    std::fprintf(stderr,
                 "MISMATCH caller %d impl %d fused %d queue %d wps %d xcd %d one %d persist %d head %d full %d robust %d prior %d iter %d nblocks %d pslots %d max_p %ld dumps %d%d%d%d: "
                 "route %d/%d fallback %d/%d lin %d/%d family %d/%d waves %d/%d fused %d/%d robust %d/%d refusal '%s' / '%s'\n",
                 (int)caller, h.pass_impl, h.fused_env, h.queue_env, h.force_wps, h.xcd_order, p.persist_one, h.persist, h.head, h.full_last_pass, h.robust_kind, h.prior_set, h.max_iter,
                 h.nblocks, h.persist_slots, h.max_p, h.stamp_path, h.span_path, h.qstat_path, h.solve_stamps, (int)got.route, (int)want.route, (int)got.fallback, (int)want.fallback, lin,
                 want.lin, (int)got.variant.family, (int)want.launch.family, got.variant.waves, want.launch.waves, got.variant.fused, want.launch.fused, got.variant.robust,
                 want.launch.robust, why.c_str(), want.refusal.c_str());
}

void walk_the_matrix() {
  const int pass_slots = 768;
  for (int impl = 0; impl <= 2; ++impl)
  for (int fused = 0; fused <= 1; ++fused)
  for (int queue = 0; queue <= 1; ++queue)
  for (int wps : {0, 3, 4})
  for (int xcd = 0; xcd <= 1; ++xcd)
  for (int one = 0; one <= 2; ++one)  // NGICP_PERSIST_ONE unset, 1, 2
  for (int persist = 0; persist <= 2; ++persist)  // off; on; on at ngicp_create and turned off by a persistent launch that failed
  for (int head = 0; head <= 1; ++head)
  for (int full = 0; full <= 1; ++full)
  for (int robust = 0; robust <= 1; ++robust)
  for (int prior = 0; prior <= 1; ++prior)
  for (int nblocks : {2 * pass_slots - 1, 2 * pass_slots, 2 * pass_slots + 1})
  for (int persist_slots : {0, 768}) {
    route::ProcessSwitches p;
    p.pass_impl = impl;
    p.fused = fused != 0;
    p.queue = queue;
    p.pass_wps = wps;
    p.xcd_order = xcd != 0;
    p.persist_one = one;
    route::HandleSwitches w;
    w.persist = persist != 0;
    w.head = head;
    w.full_last_pass = full;
    Old h{};
    h.pass_impl = impl, h.queue_env = queue, h.force_wps = wps, h.fused_env = fused != 0, h.xcd_order = xcd != 0, h.persist_one = one != 0;
    h.persist = persist == 1, h.head = head, h.full_last_pass = full, h.robust_kind = robust ? NGICP_ROBUST_HUBER : NGICP_ROBUST_NONE, h.prior_set = prior != 0;
    h.pass_slots = pass_slots, h.persist_slots = persist_slots, h.nblocks = nblocks, h.max_iter = 1, h.max_p = 11;
    route::Facts f;
    f.persist = h.persist;
    f.robust = robust != 0;
    f.prior = prior != 0;
    f.nblocks = nblocks, f.pass_slots = pass_slots, f.persist_slots = persist_slots, f.max_passes = h.max_p;
    // the hooks and the sharded pass: no dumps, no xcd order of their own, one pass whatever max_iter says
    f.caller = route::Caller::Hook;
    compare(h, f.caller, legacy_hook(h, 2 | 4), p, w, f, "linearize / compute_error");  // ngicp_linearize
    compare(h, f.caller, legacy_hook(h, 1 | 4), p, w, f, "linearize / compute_error");  // ngicp_compute_error
    f.caller = route::Caller::Sharded;
    compare(h, f.caller, legacy_sharded(h), p, w, f, "ngicp_sharded_pass");
    f.caller = route::Caller::Align;
    for (int iter = 0; iter <= 1; ++iter)
    for (long max_p : {(long)route::kMaxPersistPasses - 1, (long)route::kMaxPersistPasses})
    for (int dumps = 0; dumps < 16; ++dumps) {
      h.max_iter = iter, h.max_p = max_p;
      h.stamp_path = dumps & 1, h.span_path = dumps & 2, h.qstat_path = dumps & 4, h.solve_stamps = dumps & 8;
      f.iterating = iter > 0;
      f.max_passes = max_p;
      f.xcd_installed = h.xcd_order;
      f.dump_stamps = h.stamp_path, f.dump_span = h.span_path, f.dump_qstats = h.qstat_path, f.dump_solve = h.solve_stamps;
      compare(h, f.caller, legacy_do_align(h), p, w, f, "ngicp_align");
    }
  }
}

// ---- the readers ----
const char* const* g_env = nullptr;  // {name, value, ..., nullptr}
const char* fake_env(const char* name) {
  for (const char* const* e = g_env; e && *e; e += 2)
    if (std::strcmp(e[0], name) == 0) return e[1];
  return nullptr;
}
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      ++g_bad;                                                            \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);      \
    }                                                                     \
  } while (0)

void check_the_readers() {
  constexpr int kStageMaxGrow = 6;
  {
    g_env = nullptr;  // nothing set: the defaults
    const route::ProcessSwitches p = route::read_process_switches(fake_env);
    CHECK(p.pass_impl == 0 && !p.fused && p.queue == 0 && p.pass_wps == 0 && !p.xcd_order && p.persist_coop && p.persist_one == 0 && p.debug_solve_launch == 0);
    const route::HandleSwitches w = route::read_handle_switches(fake_env, kStageMaxGrow);
    CHECK(w.persist == 0 && w.head == 0 && w.full_last_pass == 0 && w.serial_step == 0 && w.cell_boxes == 0 && w.target_occ == 24.0 && w.voxel == 0.0 && w.chunk == 3 && w.stage_grow == 6);
  }
  {
    const char* env[] = {"NGICP_PASS_IMPL", "1", "NGICP_FUSED", "2", "NGICP_QUEUE", "1", "NGICP_PASS_WPS", "4", "NGICP_ORDER", "xcd", "NGICP_PERSIST_COOP", "0",
                         "NGICP_PERSIST_ONE", "2", "NGICP_DEBUG_SOLVE", "7", nullptr};
    g_env = env;
    const route::ProcessSwitches p = route::read_process_switches(fake_env);
    CHECK(p.pass_impl == 1 && p.fused && p.queue == 1 && p.pass_wps == 4 && p.xcd_order && !p.persist_coop && p.persist_one == 2 && p.debug_solve_launch == 7);
  }
  {
    const char* env[] = {"NGICP_FUSED", "0", "NGICP_ORDER", "XCD", "NGICP_PERSIST_COOP", "1", "NGICP_PERSIST_ONE", "0", nullptr};
    g_env = env;
    const route::ProcessSwitches p = route::read_process_switches(fake_env);
    CHECK(!p.fused);
    CHECK(!p.xcd_order);          // (a string compare: only "xcd")
    CHECK(p.persist_coop);
    CHECK(p.persist_one == 1);    // (a presence test: any value but 2 runs the route with PassArgs::persist = 1)
  }
  {
    const char* env[] = {"NGICP_PERSIST", "1", "NGICP_HEAD", "1", "NGICP_FULL_LAST_PASS", "1", "NGICP_SERIAL_STEP", "5", "NGICP_CELL_BOXES", "1", "NGICP_TARGET_OCC", "0.5",
                         "NGICP_VOXEL", "0.25", "NGICP_CHUNK", "0", "NGICP_STAGE_GROW", "99", nullptr};
    g_env = env;
    const route::HandleSwitches w = route::read_handle_switches(fake_env, kStageMaxGrow);
    CHECK(w.persist == 1 && w.head == 1 && w.full_last_pass == 1 && w.cell_boxes == 1 && w.voxel == 0.25);
    CHECK(w.serial_step == 1);    // (atoi != 0)
    CHECK(w.target_occ == 1.0);   // 0.5 -> 1.0
    CHECK(w.chunk == 1);          // 0 -> 1
    CHECK(w.stage_grow == kStageMaxGrow);
  }
  {
    const char* env[] = {"NGICP_CHUNK", "99", "NGICP_STAGE_GROW", "-3", "NGICP_TARGET_OCC", "30", "NGICP_SERIAL_STEP", "0", nullptr};
    g_env = env;
    const route::HandleSwitches w = route::read_handle_switches(fake_env, kStageMaxGrow);
    CHECK(w.chunk == 64);         // 99 -> 64
    CHECK(w.stage_grow == 0);
    CHECK(w.target_occ == 30.0);
    CHECK(w.serial_step == 0);
  }
  // the entry table: the parent's three messages, in the parent's order
  CHECK(route::entry_refusal(route::Entry::ShardedStep, true, true, true) == "ngicp_sharded_step: not available with a voxelized target (ngicp_set_voxel_resolution(h, 0) selects exact GICP)");
  CHECK(route::entry_refusal(route::Entry::AlignBatch, false, true, true) == "ngicp_align_batch: not available with a robust kernel set (ngicp_set_robust_kernel(h, NGICP_ROBUST_NONE, 0) turns it off)");
  CHECK(route::entry_refusal(route::Entry::ShardedBegin, false, false, true) == "ngicp_sharded_begin: not available with a pose prior set (ngicp_set_pose_prior(h, NULL, NULL) clears it)");
  CHECK(route::entry_refusal(route::Entry::AlignBatch, false, false, true).empty());
  CHECK(route::entry_refusal(route::Entry::VoxelAlignBatch, true, false, true).empty());
  CHECK(route::entry_refusal(route::Entry::CovsShardCommit, false, true, true).empty());
  CHECK(route::entry_refusal(route::Entry::Hook, true, true, true).empty());
}

}  // namespace

int main() {
  walk_the_matrix();
  check_the_readers();
  std::printf("cells %ld new_refusals %ld mismatches %ld\n", g_cells, g_new_refusals, g_bad);
  return g_bad == 0 ? 0 : 1;
}
