// Which pass route an alignment takes, and what each route and each entry point supports: the NGICP_* switches (each read in ONE place),
// the table of routes, choose_route, the refusals.  Host only, no HIP types: compiles with a plain C++17 compiler against include/ngicp.h
// alone (tests/cpp/route_table.cpp walks the whole decision there).  DESIGN.md "Switches and routes" is this file as a table.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/ngicp.h"

namespace route {

constexpr int kMaxPersistPasses = 2048;  // alignments with more possible passes than this take one launch per pass (the ring of views is 512 bytes per pass)

using Lookup = const char* (*)(const char*);  // std::getenv's shape: a test feeds the readers without touching the environment
inline const char* from_environment(const char* name) { return std::getenv(name); }

// ---- the switches ----
// Read once per process (switches() below: a function-local static, filled by the first call that asks): a test reaches them only through
// a child process with the variable in its environment.
struct ProcessSwitches {
  int pass_impl = 0;       // NGICP_PASS_IMPL: 1 the staged search (k_gicp_pass_st); any other non-zero value only keeps full passes
  bool fused = false;      // NGICP_FUSED: the solver in the tail of the pass launch
  int queue = 0;           // NGICP_QUEUE: resident blocks that draw their groups from a counter (k_gicp_queue)
  int pass_wps = 0;        // NGICP_PASS_WPS: 3 or 4 forces that build of the pass kernel (A/B timing only)
  bool xcd_order = false;  // NGICP_ORDER=xcd: a fixed launch order, an eighth of the groups per XCD
  bool persist_coop = true;  // NGICP_PERSIST_COOP=0: the persistent kernel by an ordinary launch (A/B timing only)
  int persist_one = 0;     // NGICP_PERSIST_ONE: 0 unset, 2 when it reads 2, 1 for anything else (PassArgs::persist of its launches)
  long debug_solve_launch = 0;  // NGICP_DEBUG_SOLVE=N: the solver launch whose stamps are kept (whether to stamp at all is debug_begin's read)
};
inline ProcessSwitches read_process_switches(Lookup env) {
  ProcessSwitches p;
  if (const char* s = env("NGICP_PASS_IMPL")) p.pass_impl = std::atoi(s);
  if (const char* s = env("NGICP_FUSED")) p.fused = std::atoi(s) != 0;
  if (const char* s = env("NGICP_QUEUE")) p.queue = std::atoi(s);
  if (const char* s = env("NGICP_PASS_WPS")) p.pass_wps = std::atoi(s);
  if (const char* s = env("NGICP_ORDER")) p.xcd_order = std::string(s) == "xcd";
  if (const char* s = env("NGICP_PERSIST_COOP")) p.persist_coop = std::atoi(s) != 0;
  if (const char* s = env("NGICP_PERSIST_ONE")) p.persist_one = std::atoi(s) == 2 ? 2 : 1;
  if (const char* s = env("NGICP_DEBUG_SOLVE")) p.debug_solve_launch = std::atol(s);
  return p;
}
inline const ProcessSwitches& switches() {
  static const ProcessSwitches p = read_process_switches(from_environment);
  return p;
}

// Read in ngicp_create and kept on the handle (ngicp::sw): monkeypatch.setenv before the handle is made reaches them.  Two of them seed
// handle state that changes later (ngicp::persist, which a persistent launch that fails clears; ngicp::voxel_size, ngicp_set_tuning).
struct HandleSwitches {
  int persist = 0;         // NGICP_PERSIST: ONE launch per alignment (k_gicp_persist)
  int head = 0;            // NGICP_HEAD: no solver launch, every block steps the optimiser at its head (k_gicp_head)
  int full_last_pass = 0;  // NGICP_FULL_LAST_PASS (diagnostic): every pass searches and linearises, whatever LmHot::lin_unneeded says
  int serial_step = 0;     // NGICP_SERIAL_STEP (A/B timing, tests): the solver steps on one lane instead of on the wave
  int cell_boxes = 0;      // NGICP_CELL_BOXES: per-cell (y,z) extents built with every index and used by the pass
  double target_occ = 24.0;  // NGICP_TARGET_OCC: mean points a random point sees in its own cell; tuned on MI355X (c2/c3/c5 workloads)
  double voxel = 0.0;      // NGICP_VOXEL: the grid's voxel edge, 0 = auto
  int chunk = 3;           // NGICP_CHUNK: (pass, solve) pairs kept in flight ahead of the solver's published progress
  int stage_grow = 6;      // NGICP_STAGE_GROW: upper limit of rings served from the LDS stage
};
inline HandleSwitches read_handle_switches(Lookup env, int stage_max_grow) {
  HandleSwitches w;
  if (const char* s = env("NGICP_PERSIST")) w.persist = std::atoi(s);
  if (const char* s = env("NGICP_HEAD")) w.head = std::atoi(s);
  if (const char* s = env("NGICP_FULL_LAST_PASS")) w.full_last_pass = std::atoi(s);
  if (const char* s = env("NGICP_SERIAL_STEP")) w.serial_step = std::atoi(s) != 0 ? 1 : 0;
  if (const char* s = env("NGICP_CELL_BOXES")) w.cell_boxes = std::atoi(s);
  if (const char* s = env("NGICP_TARGET_OCC")) w.target_occ = std::max(1.0, std::atof(s));
  if (const char* s = env("NGICP_VOXEL")) w.voxel = std::atof(s);
  if (const char* s = env("NGICP_CHUNK")) w.chunk = std::max(1, std::min(64, std::atoi(s)));
  if (const char* s = env("NGICP_STAGE_GROW")) w.stage_grow = std::max(0, std::min(stage_max_grow, std::atoi(s)));
  return w;
}

// ---- the routes (why the measured-and-rejected ones stay) ----
enum class Route { Default, Staged, Queue, Fused, Persist, PersistOne, Head };
struct RouteRow {
  Route route;
  const char* asked_by;  // the switch, as the error messages spell it
  bool robust;           // a robust instantiation exists
  bool prior;            // the pose prior is applied (the optimiser steps in lm_solve_body)
  bool lin_unneeded;     // its pass honours LmHot::lin_unneeded (K4-only passes)
  bool own_solver;       // a solver launch of its own behind every pass
};
constexpr RouteRow kRoutes[] = {  // (behind the default: in the order the refusals look at the switches)
    {Route::Default, "", true, true, true, true},                          // the walks in global memory (k_gicp_pass)
    {Route::Staged, "NGICP_PASS_IMPL=1", false, true, false, true},        // the staged search (k_gicp_pass_st)
    {Route::Fused, "NGICP_FUSED", false, true, true, false},               // k_gicp_pass<.., true>: the last block of the pass steps
    {Route::Queue, "NGICP_QUEUE", false, true, false, true},               // the queue grid (k_gicp_queue)
    {Route::Persist, "NGICP_PERSIST", false, true, false, false},          // the persistent kernel (k_gicp_persist)
    {Route::Head, "NGICP_HEAD", false, false, false, false},               // the step at the head of the next pass (k_gicp_head)
    {Route::PersistOne, "NGICP_PERSIST_ONE", false, true, false, false},   // the persistent kernel's code, one launch per pass
};
constexpr const RouteRow& row(Route r) {
  for (const RouteRow& x : kRoutes)
    if (x.route == r) return x;
  return kRoutes[0];
}

// Who asks: ngicp_align; the hooks (ngicp_linearize, ngicp_compute_error: one pass on the handle's state); ngicp_sharded_begin / _pass.
enum class Caller { Align, Hook, Sharded };

// The facts of one alignment (or one hook pass) the choice depends on.  The hooks and the sharded pass have no dumps and no xcd order.
struct Facts {
  Caller caller = Caller::Align;
  int persist = 0;         // ngicp::persist now: the switch, unless a persistent launch on this handle has failed
  bool robust = false, prior = false;
  bool iterating = true;   // max_iter > 0
  int nblocks = 1, pass_slots = 1, persist_slots = 0;
  long max_passes = 0;
  bool xcd_installed = false;
  bool dump_stamps = false, dump_span = false, dump_qstats = false, dump_solve = false;
};

enum class Family { Walks, Staged, Queue };
struct Variant {           // the pass kernel of a launch-per-pass route
  Family family = Family::Walks;
  int waves = 3;
  bool fused = false, robust = false;
};
struct Choice {
  Route route;             // the route to try
  Route fallback;          // the route to take if the persistent launch declines (route itself where route is not Persist)
  Variant variant;         // of the launch-per-pass route among the two (Default, Staged, Queue, Fused); untouched otherwise
};

// The precedence, from the top: Persist, Head (both need `plain`: the default pass, unfused, in the measured launch order, without per-block
// dumps), PersistOne (whatever NGICP_PASS_IMPL says), then one launch per pass: Staged, Queue, Fused, the robust build, the default.
inline Choice choose_route(const ProcessSwitches& p, const HandleSwitches& w, const Facts& f) {
  const bool align = f.caller == Caller::Align, hook = f.caller == Caller::Hook;
  const bool fused = align && p.fused && p.pass_impl == 0;
  const bool ring_fits = f.persist_slots > 0 && f.max_passes + 1 <= kMaxPersistPasses;
  const bool plain = align && f.iterating && p.pass_impl == 0 && !fused && !f.xcd_installed && !f.dump_span && !f.dump_qstats && !f.dump_solve;
  Choice c{Route::Default, Route::Default, Variant{}};
  Variant& v = c.variant;
  v.waves = p.pass_wps ? (p.pass_wps == 4 ? 4 : 3) : (f.nblocks > 2 * f.pass_slots ? 4 : 3);
  if (w.head && plain && f.nblocks <= 2 * f.pass_slots) {  // (grids of more rounds: the head's few microseconds are paid once per round)
    c.fallback = Route::Head;
  } else if (align && p.persist_one && ring_fits) {
    c.fallback = Route::PersistOne;
  } else if (p.pass_impl == 1) {
    c.fallback = Route::Staged;
    v.family = Family::Staged;
    if (!p.pass_wps) v.waves = 4;  // (128 VGPRs either way; the 4-wave build's smaller tables leave room for a fourth block per CU)
  } else if (p.queue && !fused && !hook && !f.dump_stamps && !f.dump_span && !f.dump_qstats) {  // (the hooks' mode bit 2 excludes it)
    c.fallback = Route::Queue;
    v.family = Family::Queue;
  } else if (fused) {
    c.fallback = Route::Fused;
    v.fused = true;
  } else {
    v.robust = f.robust;
  }
  c.route = (f.persist && plain && ring_fits && !f.dump_stamps) ? Route::Persist : c.fallback;
  if (c.fallback == Route::Head || c.fallback == Route::PersistOne) v = Variant{};
  return c;
}

// Whether the switch that asks for route r is SET and this caller's pass obeys it: the hooks' pass obeys NGICP_PASS_IMPL alone, the sharded
// pass that and NGICP_QUEUE.  What the switches that are set support is decided by this, not by the route the alignment ends up on.
inline bool asked(Route r, const ProcessSwitches& p, const HandleSwitches& w, const Facts& f) {
  const bool align = f.caller == Caller::Align;
  switch (r) {
    case Route::Staged: return p.pass_impl == 1;
    case Route::Queue: return f.caller != Caller::Hook && p.queue != 0;
    case Route::Fused: return align && p.fused;
    case Route::Persist: return align && f.persist != 0;
    case Route::Head: return align && w.head != 0;
    case Route::PersistOne: return align && p.persist_one != 0;
    default: return false;
  }
}

// Whether the passes honour LmHot::lin_unneeded: not under a switch whose route keeps full passes, even where the alignment ends up on the
// default route, and not under NGICP_FULL_LAST_PASS or any NGICP_PASS_IMPL but 0.  (The hooks name their pass's mode themselves.)
inline bool honours_lin_unneeded(const ProcessSwitches& p, const HandleSwitches& w, const Facts& f) {
  if (f.caller == Caller::Hook || w.full_last_pass || p.pass_impl != 0) return false;
  for (const RouteRow& r : kRoutes)
    if (asked(r.route, p, w, f) && !r.lin_unneeded) return false;
  return true;
}

// What an alignment with a robust kernel or a pose prior is refused for, or "": by the switches that are SET, in kRoutes' order (a pass that
// silently ignored the kernel, or a step that skipped the prior, would be a wrong answer, not a slower one).  The sharded entries refuse both
// settings outright (kEntries); of the hooks' one switch, NGICP_PASS_IMPL=1, the row refuses the robust kernel alone.
inline std::string refusal(const ProcessSwitches& p, const HandleSwitches& w, const Facts& f, const char* entry) {
  if (f.caller == Caller::Sharded) return {};
  const bool hook = f.caller == Caller::Hook;
  if (f.robust)
    for (const RouteRow& r : kRoutes)
      if (asked(r.route, p, w, f) && !r.robust)
        return std::string(entry) + ": the robust kernel has no instantiation of the pass variant " + r.asked_by + " selects" +
               (hook ? "" : " (unset it, or ngicp_set_robust_kernel(h, NGICP_ROBUST_NONE, 0))");
  if (f.prior)
    for (const RouteRow& r : kRoutes)
      if (asked(r.route, p, w, f) && !r.prior)
        return std::string(entry) + ": the pose prior is not applied by the route " + r.asked_by + " selects (unset it, or ngicp_set_pose_prior(h, NULL, NULL))";
  return {};
}

// ---- what each entry point refuses outright ----
enum class Entry { AlignBatch, VoxelAlignBatch, ShardedBegin, ShardedPass, ShardedStep, ShardedFinish, CovsShardBegin, CovsShardCompute, CovsShardCommit, Hook };
struct EntryRow {
  Entry entry;
  const char* name;
  bool voxelized, robust, prior;  // refused with a voxelized target / a robust kernel / a pose prior set
};
constexpr EntryRow kEntries[] = {
    {Entry::AlignBatch, "ngicp_align_batch", true, true, false},
    {Entry::VoxelAlignBatch, "ngicp_voxel_align_batch", false, true, false},
    // the sharded entries step on all-reduced sums, outside lm_solve_body's row: no robust weights, no prior
    {Entry::ShardedBegin, "ngicp_sharded_begin", true, true, true},
    {Entry::ShardedPass, "ngicp_sharded_pass", true, true, true},
    {Entry::ShardedStep, "ngicp_sharded_step", true, true, true},
    {Entry::ShardedFinish, "ngicp_sharded_finish", true, true, true},
    {Entry::CovsShardBegin, "ngicp_covs_shard_begin", true, false, false},
    {Entry::CovsShardCompute, "ngicp_covs_shard_compute", true, false, false},
    {Entry::CovsShardCommit, "ngicp_covs_shard_commit", true, false, false},
    {Entry::Hook, "linearize / compute_error", false, false, false},  // (both modes, robust and prior: only refusal() above)
};
inline std::string entry_refusal(Entry e, bool voxelized, bool robust, bool prior) {
  for (const EntryRow& r : kEntries) {
    if (r.entry != e) continue;
    if (r.voxelized && voxelized) return std::string(r.name) + ": not available with a voxelized target (ngicp_set_voxel_resolution(h, 0) selects exact GICP)";
    if (r.robust && robust) return std::string(r.name) + ": not available with a robust kernel set (ngicp_set_robust_kernel(h, NGICP_ROBUST_NONE, 0) turns it off)";
    if (r.prior && prior) return std::string(r.name) + ": not available with a pose prior set (ngicp_set_pose_prior(h, NULL, NULL) clears it)";
  }
  return {};
}

}  // namespace route
