// gr_fit_exec.cpp — the fit step's per-view schedule as native host code (gr_fit_views, include/gr_hip.h).
//
// The reference fit loop renders its views one after another (fit_multiview_stub.py:277-310).  The
// multi-GPU driver (3dgaussian_amd/fit_multiview.py) runs the same work on several HIP streams with the
// views' preparations ahead on a stream of their own; this file is that schedule in C++, so a step costs
// the host a few microseconds per launch instead of the Python driver's per-view interpreter work
// (the small-view configs and the per-rank share of a multi-GPU step are host-bound in Python).
//
// Only the public C ABI (gr_fwd_prepare_views_async, gr_fwd_render_l1, gr_bwd_splat, gr_gather_view,
// gr_reduce_sums, gr_density_stats, gr_camera_grads_sums, gr_fwd_render, gr_bwd_fit_gather, gr_bwd_fit_ssim_gather) and the HIP runtime are used.
// Workspaces are the executor's own, kept across steps and reused only in stream order: each render stream owns its view workspace
// (bins, forward scratch, backward workspace, saved sums) and a ring of per-view sums for its reduction
// batch; the geoms are a ring of slots written on the preparation stream, a slot being rewritten only
// after the preparation stream has waited for the event recorded behind its last reader.  A buffer that
// must grow is replaced after its stream has drained (rare: the first step, a densify).
// The schedule (streams, preparation groups, reduction batches) is exactly fit_multiview._views_direct's,
// so both give bit-identical losses and gradients (tests/test_fit_exec_gpu.py).
// gr_eval_views, gr_eval_views_cc, gr_eval_views_masked, gr_contrib_views and gr_error_views are the same schedule without
// a backward (a render-only pass): per view gr_fwd_render (saved sums only) and the pass's calls on them (gr_eval_view into
// the view's row of metrics, for gr_eval_views_cc followed by gr_cc_fit_view and gr_eval_view_cc, for gr_eval_views_masked
// by gr_eval_view_masked, into the same row; gr_contrib_view or
// gr_error_view, every view into the caller's one buffer), with one pass workspace per render stream; a pass writes
// nothing but those workspaces and the caller's output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/gr_hip.h"

extern "C" gr_status gr_exec_set_error(gr_status st, const char* msg);  // gr_hip.hip: thread-local message

namespace {

struct Sched {
  int ns;                              // streams used
  std::vector<std::deque<int>> sizes;  // per stream: its reduction batch sizes, in order
};

// fit_multiview._views_direct's batches: stream k's views in near-equal batches of at most reduce_batch,
// the last one reduce_tail views (when 0 < tail < the stream's view count).
Sched schedule(int views, const gr_fit_config& c) {
  Sched s;
  s.ns = std::max(1, std::min(c.num_streams, views));
  s.sizes.resize(s.ns);
  for (int k = 0; k < s.ns; ++k) {
    const int p = views > k ? (views - k + s.ns - 1) / s.ns : 0;
    const int tail = (c.reduce_tail > 0 && c.reduce_tail < p) ? c.reduce_tail : 0;
    const int nb = std::max(1, (p - tail + c.reduce_batch - 1) / c.reduce_batch);
    for (int b = 0; b < nb; ++b) s.sizes[k].push_back((p - tail) / nb + (b < (p - tail) % nb ? 1 : 0));
    if (tail) s.sizes[k].push_back(tail);
  }
  return s;
}

}  // namespace

// A device buffer that grows: replaced (old one freed after `s` has drained) when a request exceeds it.
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t fit(size_t bytes, hipStream_t s) {
    if (bytes <= cap) return hipSuccess;
    if (p) {
      hipError_t e = hipStreamSynchronize(s);
      if (e == hipSuccess) e = hipFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      cap = 0;
    }
    const size_t want = bytes + bytes / 8 + (1u << 20);  // headroom: pair counts drift from step to step
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct StreamWs {  // one render stream's buffers
  Buf bins, scratch, ws, saved;
  Buf pass;                      // a render-only pass's workspace: the metrics' or moments' partial sums, or the pairs' values
  Buf cam;                       // gr_executor_camera_grads: a batch's camera-gradient partials
  std::vector<Buf> sums, sums3;  // one per view of a reduction batch (sums3: the depth-loss path's depth sums)
};

struct GeomSlot {
  Buf buf;
  hipEvent_t free_ev = nullptr;  // recorded behind the slot's last reader
  bool pending = false;          // free_ev recorded and not yet waited for by the preparation stream
};

struct gr_executor {
  int device = 0;
  hipStream_t prep = nullptr;
  std::vector<hipStream_t> side;   // render streams 1..; stream 0 is the caller's
  std::vector<hipEvent_t> groups;  // one event per preparation group (reused across steps)
  hipEvent_t in = nullptr;
  std::vector<hipEvent_t> done;    // side streams' ends
  gr_plan* plans = nullptr;        // pinned, mapped: one plan per view (written by the preparation kernels)
  int plans_cap = 0;
  std::vector<StreamWs> ws;        // per render stream
  std::vector<GeomSlot> geoms;     // ring of geom slots
  std::vector<hipStream_t> last;   // the previous call's render streams 1.. and preparation stream
  float* const* stats = nullptr;   // gr_executor_density_stats: one [n][2] buffer per render stream, or none
  float* cams = nullptr;           // gr_executor_camera_grads: [num_views][GR_CAMERA_GRADS] rows (view j -> row j), or none
};

#define GR_EXEC_TRY(expr)                                                            \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) return gr_exec_set_error(GR_ERR_HIP, hipGetErrorString(e_)); \
  } while (0)
#define GR_EXEC_CALL(expr)          \
  do {                              \
    gr_status s_ = (expr);          \
    if (s_ != GR_OK) return s_;     \
  } while (0)

// What is done with each view: the fit (loss, backward, reductions) or a render-only pass (no losses, accumulators or
// statistics: per view the render and one call that reads its saved sums).
struct Pass {
  enum Kind { fit, eval, contrib, error, eval_cc, eval_masked } kind = fit;
  float* out = nullptr;  // eval, eval_cc, eval_masked: the views' rows; contrib, error: the one per-Gaussian buffer
  float ridge = 0.0f;    // eval_cc: gr_cc_fit_view's
  bool fwd_only() const { return kind != fit; }

  // A render-only pass, stated once per kind.  The floats of a view's row in `out` (0: the one per-Gaussian buffer):
  int row_width() const {
    switch (kind) {
      case eval: return GR_EVAL_METRICS;
      case eval_cc: return GR_EVAL_CC_ROW;
      case eval_masked: return GR_EVAL_METRICS + GR_EVAL_MASK_METRICS;
      default: return 0;
    }
  }
  // the workspace of a view's calls (one after another on the view's stream, so the largest of their sizes):
  size_t ws_bytes(const gr_view* v, int n, const gr_plan* plan) const {
    switch (kind) {
      case eval_cc: return std::max(gr_eval_ws_bytes(v), gr_cc_ws_bytes(v));
      case eval_masked: return std::max(gr_eval_ws_bytes(v), gr_eval_mask_ws_bytes(v));
      case contrib: return gr_contrib_ws_bytes(v, n, plan);
      case error: return gr_error_ws_bytes(v, n, plan);
      default: return gr_eval_ws_bytes(v);
    }
  }
  // and the calls on view j's saved sums (W.saved, in W.pass): a metric pass begins with gr_eval_view into the row's
  // first three columns, then the kind's own into the columns behind; contrib, error: atomic maxima into `out`.
  gr_status on_saved(int j, const gr_fit_target& t, int n, const gr_plan* plan, const void* geom, const void* bins,
                     const StreamWs& W, void* s) const {
    const gr_view* v = &t.view;
    const float* saved = (const float*)W.saved.p;
    float* row = out + (size_t)row_width() * j;
    float* own = row + GR_EVAL_METRICS;
    if (row_width() > 0) GR_EXEC_CALL(gr_eval_view(v, saved, t.target_rgb, row, W.pass.p, W.pass.cap, s));
    switch (kind) {
      case eval_cc:  // (the transform behind the corrected metrics)
        GR_EXEC_CALL(gr_cc_fit_view(v, saved, t.target_rgb, ridge, own + GR_EVAL_METRICS, W.pass.p, W.pass.cap, s));
        return gr_eval_view_cc(v, saved, t.target_rgb, own + GR_EVAL_METRICS, own, W.pass.p, W.pass.cap, s);
      case eval_masked: return gr_eval_view_masked(v, saved, t.target_rgb, t.target_mask, own, W.pass.p, W.pass.cap, s);
      case contrib: return gr_contrib_view(v, n, plan, geom, bins, saved, out, W.pass.p, W.pass.cap, s);
      case error: return gr_error_view(v, n, plan, geom, bins, saved, t.target_rgb, out, W.pass.p, W.pass.cap, s);
      default: return GR_OK;
    }
  }
};

// A call's operands beside its views: the activated parameters, the loss terms and where the losses and the streams'
// gradient accumulators go (a render-only pass has neither).
struct Params {
  const float *means = nullptr, *scales = nullptr, *colors = nullptr;
  int color_dim = 3;
  const float* opacities = nullptr;
};
struct Operands {
  int n = 0;
  Params p;
  float w_sil = 0.0f, w_depth = 0.0f, g_scale = 1.0f, w_dssim = 0.0f;  // w_dssim > 0: the D-SSIM form
  float* losses = nullptr;
  float* const* acc = nullptr;
};

static gr_status fit_views_on_device(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views,
                                     const Operands& op, void* stream, Pass pass = {});
static gr_status enqueue_views(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views,
                               const Operands& op, const Sched& sc, const std::vector<hipStream_t>& st, hipStream_t prep,
                               bool depth, int nslots, int& ngroups, Pass pass);

extern "C" {

gr_status gr_executor_create(int device, gr_executor** out) {
  if (!out) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_executor_create: null output");
  *out = nullptr;
  int cur = 0;
  GR_EXEC_TRY(hipGetDevice(&cur));
  GR_EXEC_TRY(hipSetDevice(device));
  gr_executor* ex = new gr_executor();
  ex->device = device;
  // streams are made on first use, and only when the caller passes none (stream creation order decides the
  // hardware queue each lands on)
  hipError_t e = hipEventCreateWithFlags(&ex->in, hipEventDisableTiming);
  (void)hipSetDevice(cur);
  if (e != hipSuccess) {
    gr_executor_destroy(ex);
    return gr_exec_set_error(GR_ERR_HIP, hipGetErrorString(e));
  }
  *out = ex;
  return GR_OK;
}

void gr_executor_destroy(gr_executor* ex) {
  if (!ex) return;
  if (ex->prep) (void)hipStreamSynchronize(ex->prep);
  for (hipStream_t s : ex->side) {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  (void)hipDeviceSynchronize();  // no queued work still uses the executor's buffers
  for (auto& w : ex->ws) {
    w.bins.release();
    w.scratch.release();
    w.ws.release();
    w.saved.release();
    w.pass.release();
    w.cam.release();
    for (auto& b : w.sums) b.release();
    for (auto& b : w.sums3) b.release();
  }
  for (auto& g : ex->geoms) {
    g.buf.release();
    if (g.free_ev) (void)hipEventDestroy(g.free_ev);
  }
  for (hipEvent_t e : ex->groups) (void)hipEventDestroy(e);
  for (hipEvent_t e : ex->done) (void)hipEventDestroy(e);
  if (ex->in) (void)hipEventDestroy(ex->in);
  if (ex->prep) (void)hipStreamDestroy(ex->prep);
  if (ex->plans) (void)hipHostFree(ex->plans);
  delete ex;
}

static gr_status fit_views_checked(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views,
                                   const Operands& op, void* stream) {
  if (!ex || !cfg || (num_views > 0 && (!views || !op.losses || !op.acc)))
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: null argument");
  // every batch of a stream (its last one holds reduce_tail views) and every preparation group must fit the
  // fixed-size view arrays of gr_reduce_sums / gr_fwd_prepare_views_async (and the per-stream sums ring)
  if (cfg->num_streams < 1 || cfg->prep_ahead < 1 || cfg->prep_group < 1 || cfg->prep_group > GR_PREPARE_MAX_VIEWS ||
      cfg->prep_first < 1 || cfg->prep_first > GR_PREPARE_MAX_VIEWS || cfg->reduce_batch < 1 ||
      cfg->reduce_batch > GR_REDUCE_MAX_VIEWS || cfg->reduce_tail < 0 || cfg->reduce_tail > cfg->reduce_batch)
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: configuration out of range");
  if (num_views == 0 || op.n <= 0) return GR_OK;
  if (cfg->caps && !cfg->overflow) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: caps without overflow");
  const bool depth = views[0].target_depth != nullptr;  // the depth-loss path (one form per call)
  for (int j = 0; j < num_views; ++j) {
    if ((views[j].target_depth != nullptr) != depth)
      return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: every view or none has a depth target");
    if (!views[j].target_rgb) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: null target");
  }
  // the executor's streams, events and buffers belong to its device: make it current for this call
  int prev_dev = 0;
  GR_EXEC_TRY(hipGetDevice(&prev_dev));
  GR_EXEC_TRY(hipSetDevice(ex->device));
  const gr_status st = fit_views_on_device(ex, cfg, num_views, views, op, stream);
  (void)hipSetDevice(prev_dev);
  return st;
}

gr_status gr_executor_density_stats(gr_executor* ex, float* const* stats_per_stream) {
  if (!ex) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_executor_density_stats: null executor");
  ex->stats = stats_per_stream;
  return GR_OK;
}

gr_status gr_executor_camera_grads(gr_executor* ex, float* d_cameras) {
  if (!ex) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_executor_camera_grads: null executor");
  ex->cams = d_cameras;
  return GR_OK;
}

gr_status gr_fit_views(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                       const float* means, const float* scales, const float* colors, int color_dim,
                       const float* opacities, float w_sil, float w_depth, float g_scale, float* losses,
                       float* const* acc, void* stream) {
  return fit_views_checked(ex, cfg, num_views, views,
                           {n, {means, scales, colors, color_dim, opacities}, w_sil, w_depth, g_scale, 0.0f, losses, acc},
                           stream);
}

gr_status gr_fit_views_ssim(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                            const float* means, const float* scales, const float* colors, int color_dim,
                            const float* opacities, float w_sil, float w_depth, float g_scale, float w_dssim,
                            float* losses, float* const* acc, void* stream) {
  if (!(w_dssim >= 0.0f && w_dssim <= 1.0f))
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views_ssim: w_dssim must be in [0, 1]");
  return fit_views_checked(ex, cfg, num_views, views,
                           {n, {means, scales, colors, color_dim, opacities}, w_sil, w_depth, g_scale, w_dssim, losses, acc},
                           stream);
}

// A render-only pass's entry point: its checks (`name` in each message) and the schedule on the executor's device.
// op: n and the parameters (no loss terms, losses or accumulators).
static gr_status pass_views_checked(const char* name, Pass pass, gr_executor* ex, const gr_fit_config* cfg, int num_views,
                                    const gr_fit_target* views, const Operands& op, void* stream) {
  const std::string who = name;
  if (!ex || !cfg || (num_views > 0 && (!views || !pass.out)))
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, (who + ": null argument").c_str());
  if (cfg->num_streams < 1 || cfg->prep_ahead < 1 || cfg->prep_group < 1 || cfg->prep_group > GR_PREPARE_MAX_VIEWS ||
      cfg->prep_first < 1 || cfg->prep_first > GR_PREPARE_MAX_VIEWS)
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, (who + ": configuration out of range").c_str());
  if (cfg->caps)
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, (who + ": device-side sizing (caps) is not supported").c_str());
  if (num_views <= 0 || op.n <= 0) return GR_OK;
  for (int j = 0; pass.kind != Pass::contrib && j < num_views; ++j)
    if (!views[j].target_rgb) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, (who + ": null target").c_str());
  for (int j = 0; pass.kind == Pass::eval_masked && j < num_views; ++j)
    if (!views[j].target_mask) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, (who + ": null mask").c_str());
  gr_fit_config c = *cfg;  // no reductions: the batch settings are ignored
  c.reduce_batch = 1;
  c.reduce_tail = 0;
  int prev_dev = 0;
  GR_EXEC_TRY(hipGetDevice(&prev_dev));
  GR_EXEC_TRY(hipSetDevice(ex->device));
  const gr_status st = fit_views_on_device(ex, &c, num_views, views, op, stream, pass);
  (void)hipSetDevice(prev_dev);
  return st;
}

gr_status gr_eval_views(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                        const float* means, const float* scales, const float* colors, int color_dim, const float* opacities,
                        float* metrics, void* stream) {
  return pass_views_checked("gr_eval_views", {Pass::eval, metrics}, ex, cfg, num_views, views,
                            {n, {means, scales, colors, color_dim, opacities}}, stream);
}

gr_status gr_eval_views_cc(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                           const float* means, const float* scales, const float* colors, int color_dim,
                           const float* opacities, float ridge, float* rows, void* stream) {
  if (!(ridge > 0.0f) || !(ridge <= 3.402823466e38f))  // (as gr_cc_fit_view, before anything is enqueued)
    return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_eval_views_cc: ridge must be positive and finite");
  return pass_views_checked("gr_eval_views_cc", {Pass::eval_cc, rows, ridge}, ex, cfg, num_views, views,
                            {n, {means, scales, colors, color_dim, opacities}}, stream);
}

gr_status gr_eval_views_masked(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                               const float* means, const float* scales, const float* colors, int color_dim,
                               const float* opacities, float* metrics, void* stream) {
  return pass_views_checked("gr_eval_views_masked", {Pass::eval_masked, metrics}, ex, cfg, num_views, views,
                            {n, {means, scales, colors, color_dim, opacities}}, stream);
}

gr_status gr_contrib_views(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                           const float* means, const float* scales, const float* colors, int color_dim,
                           const float* opacities, float* peak, void* stream) {
  return pass_views_checked("gr_contrib_views", {Pass::contrib, peak}, ex, cfg, num_views, views,
                            {n, {means, scales, colors, color_dim, opacities}}, stream);
}

gr_status gr_error_views(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views, int n,
                         const float* means, const float* scales, const float* colors, int color_dim,
                         const float* opacities, float* err, void* stream) {
  return pass_views_checked("gr_error_views", {Pass::error, err}, ex, cfg, num_views, views,
                            {n, {means, scales, colors, color_dim, opacities}}, stream);
}

}  // extern "C"

static gr_status fit_views_on_device(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views,
                                     const Operands& op, void* stream, Pass pass) {
  const bool fwd_only = pass.fwd_only();
  const bool depth = !fwd_only && views[0].target_depth != nullptr;
  const Sched sc = schedule(num_views, *cfg);
  const int ns = sc.ns;
  for (int k = 0; !fwd_only && k < ns; ++k)
    for (int q = 0; q < 4; ++q)
      if (!op.acc[4 * k + q]) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: null accumulator");
  for (int k = 0; !fwd_only && ex->stats && k < ns; ++k)
    if (!ex->stats[k]) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: null density stats buffer");
  hipStream_t main = (hipStream_t)stream;
  // streams, events and the plan array, grown on demand and kept
  while (!cfg->render_streams && (int)ex->side.size() < ns - 1) {
    hipStream_t s;
    GR_EXEC_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    ex->side.push_back(s);
  }
  while ((int)ex->done.size() < ns - 1) {
    hipEvent_t e;
    GR_EXEC_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ex->done.push_back(e);
  }
  if ((int)ex->ws.size() < ns) ex->ws.resize(ns);
  for (int k = 0; !fwd_only && k < ns; ++k)
    if ((int)ex->ws[k].sums.size() < cfg->reduce_batch) {
      ex->ws[k].sums.resize(cfg->reduce_batch);
      ex->ws[k].sums3.resize(cfg->reduce_batch);
    }
  // geom slots: the views prepared ahead, the ones rendering on every stream, and a margin
  const int nslots = cfg->prep_ahead + cfg->prep_group + ns + 2;
  while ((int)ex->geoms.size() < nslots) {
    ex->geoms.emplace_back();
    GR_EXEC_TRY(hipEventCreateWithFlags(&ex->geoms.back().free_ev, hipEventDisableTiming));
  }
  const int max_groups = num_views + 1;
  while ((int)ex->groups.size() < max_groups) {
    hipEvent_t e;
    GR_EXEC_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ex->groups.push_back(e);
  }
  if (ex->plans_cap < num_views) {
    if (ex->plans) {
      GR_EXEC_TRY(hipDeviceSynchronize());  // no preparation of an earlier step still writes them
      GR_EXEC_TRY(hipHostFree(ex->plans));
    }
    GR_EXEC_TRY(hipHostMalloc((void**)&ex->plans, sizeof(gr_plan) * num_views, hipHostMallocMapped));
    ex->plans_cap = num_views;
  }
  std::vector<hipStream_t> st(ns);
  st[0] = main;
  for (int k = 1; k < ns; ++k) {
    st[k] = cfg->render_streams ? (hipStream_t)cfg->render_streams[k - 1] : ex->side[k - 1];
    if (!st[k]) return gr_exec_set_error(GR_ERR_INVALID_ARGUMENT, "gr_fit_views: null render stream");
  }
  if (!cfg->prep_stream && !ex->prep) GR_EXEC_TRY(hipStreamCreateWithFlags(&ex->prep, hipStreamNonBlocking));
  const hipStream_t prep = cfg->prep_stream ? (hipStream_t)cfg->prep_stream : ex->prep;
  // the workspaces of every render stream (stream 0's on the caller's stream) and the geom slots were last used on
  // the previous call's streams: when any of them changes, those finish first
  std::vector<hipStream_t> now(st.begin(), st.end());
  now.push_back(prep);
  if (!ex->last.empty() && ex->last != now)
    for (hipStream_t s : ex->last) GR_EXEC_TRY(hipStreamSynchronize(s));
  ex->last = now;
  // everything starts after the caller's stream (the activations)
  GR_EXEC_TRY(hipEventRecord(ex->in, main));
  GR_EXEC_TRY(hipStreamWaitEvent(prep, ex->in, 0));
  for (int k = 1; k < ns; ++k) GR_EXEC_TRY(hipStreamWaitEvent(st[k], ex->in, 0));
  // From here work is enqueued on the executor's streams: whatever happens below, the caller's stream is ordered
  // after all of it before this returns (an error part-way must not let the caller free buffers still in use).
  int ngroups = 0;
  auto join = [&]() {
    for (int k = 1; k < ns; ++k)
      if (hipEventRecord(ex->done[k - 1], st[k]) != hipSuccess || hipStreamWaitEvent(main, ex->done[k - 1], 0) != hipSuccess)
        (void)hipStreamSynchronize(st[k]);
    if (hipEventRecord(ex->groups[ngroups], prep) != hipSuccess || hipStreamWaitEvent(main, ex->groups[ngroups], 0) != hipSuccess)
      (void)hipStreamSynchronize(prep);
  };
  const gr_status status = enqueue_views(ex, cfg, num_views, views, op, sc, st, prep, depth, nslots, ngroups, pass);
  join();
  return status;
}

static gr_status enqueue_views(gr_executor* ex, const gr_fit_config* cfg, int num_views, const gr_fit_target* views,
                               const Operands& op, const Sched& sc, const std::vector<hipStream_t>& st, hipStream_t prep,
                               bool depth, int nslots, int& ngroups, Pass pass) {
  const int n = op.n;
  const Params& p = op.p;
  const bool fwd_only = pass.fwd_only();  // no backward, no reductions
  const int ns = sc.ns;
  const bool sized = cfg->caps != nullptr;  // device-side sizing: the plans are capacities, nothing to wait for
  const size_t geom_bytes = gr_geom_bytes(n);
  std::vector<void*> geom(num_views, nullptr);
  std::vector<int> slot_of(num_views, -1);
  std::vector<int> group_of(num_views, -1);
  int next_prep = 0;
  auto prepare_upto = [&](int j) -> gr_status {  // views [next_prep, j] prepared (whole groups)
    while (next_prep < num_views && next_prep <= j) {
      const int g0 = next_prep, cnt = std::min(num_views - g0, g0 == 0 ? cfg->prep_first : cfg->prep_group);
      gr_view vs[GR_PREPARE_MAX_VIEWS];
      void* gs[GR_PREPARE_MAX_VIEWS];
      gr_plan* ps[GR_PREPARE_MAX_VIEWS];
      for (int q = 0; q < cnt; ++q) {
        const int sl = (g0 + q) % nslots;
        GeomSlot& g = ex->geoms[sl];
        if (g.pending) {  // its previous view's readers first (stream order on the preparation stream)
          GR_EXEC_TRY(hipStreamWaitEvent(prep, g.free_ev, 0));
          g.pending = false;
        }
        GR_EXEC_TRY(g.buf.fit(geom_bytes, prep));
        geom[g0 + q] = g.buf.p;
        slot_of[g0 + q] = sl;
        vs[q] = views[g0 + q].view;
        gs[q] = geom[g0 + q];
        ps[q] = sized ? (cfg->observed ? &cfg->observed[g0 + q] : nullptr) : &ex->plans[g0 + q];
        group_of[g0 + q] = ngroups;
      }
      if (sized)
        GR_EXEC_CALL(gr_fwd_prepare_views_sized(cnt, vs, n, p.means, p.scales, p.colors, p.color_dim, p.opacities, gs,
                                                geom_bytes, cfg->caps + g0, ps, cfg->overflow, prep));
      else
        GR_EXEC_CALL(gr_fwd_prepare_views_async(cnt, vs, n, p.means, p.scales, p.colors, p.color_dim, p.opacities, gs,
                                                geom_bytes, ps, prep));
      GR_EXEC_TRY(hipEventRecord(ex->groups[ngroups], prep));
      ++ngroups;
      next_prep = g0 + cnt;
    }
    return GR_OK;
  };

  struct Pending {
    int j;  // the view's index in the call (its camera-gradient row)
    gr_view view;
    float* sums;
    float* sums3;  // depth sums (depth-loss path) or null
  };
  // a slot's previous view must have been waited for before the slot is refilled: with nslots > prep_ahead
  // + prep_group + ns the view a slot last held was rendered (and its free event recorded) before the
  // preparation that refills it is enqueued
  std::vector<std::vector<Pending>> pending(ns);
  std::vector<std::deque<int>> sizes = sc.sizes;
  std::vector<int> started(ns, 0);
  const size_t sums_bytes = gr_view_sums_floats(n) * sizeof(float);
  auto reduce_pending = [&](int k) -> gr_status {
    if (pending[k].empty()) return GR_OK;
    gr_sums_view b[GR_REDUCE_MAX_VIEWS];
    const int nb = (int)pending[k].size();
    for (int q = 0; q < nb; ++q) {
      b[q].view = pending[k][q].view;
      b[q].sums = pending[k][q].sums;
      b[q].sums3 = pending[k][q].sums3;
    }
    float* const* acc = op.acc + 4 * k;
    GR_EXEC_CALL(gr_reduce_sums(nb, b, n, p.means, p.scales, p.colors, p.color_dim, p.opacities, acc[0], acc[1], acc[2],
                                acc[3], started[k], st[k]));
    if (ex->stats)  // the batch's density statistics beside its chain rule (gr_executor_density_stats)
      GR_EXEC_CALL(gr_density_stats(nb, b, n, p.means, p.scales, p.opacities, 1.0f / op.g_scale, ex->stats[k], st[k]));
    if (ex->cams) {  // the batch's camera gradients, view j into row j (gr_executor_camera_grads)
      float* rows[GR_REDUCE_MAX_VIEWS];
      for (int q = 0; q < nb; ++q) rows[q] = ex->cams + (size_t)GR_CAMERA_GRADS * pending[k][q].j;
      Buf& cw = ex->ws[k].cam;
      GR_EXEC_TRY(cw.fit(gr_camera_grads_ws_bytes(n, nb), st[k]));
      GR_EXEC_CALL(gr_camera_grads_sums(nb, b, n, p.means, p.scales, p.colors, p.color_dim, p.opacities, rows, cw.p, cw.cap,
                                        st[k]));
    }
    pending[k].clear();
    started[k] = 1;
    return GR_OK;
  };

  // the first two groups, then one more after each render (fit_multiview._prep_groups): the first render is
  // enqueued before the later groups
  GR_EXEC_CALL(prepare_upto(std::min(cfg->prep_first, cfg->prep_ahead - 1)));
  for (int j = 0; j < num_views; ++j) {
    const int k = j % ns;
    hipStream_t s = st[k];
    GR_EXEC_CALL(prepare_upto(j));
    const hipEvent_t ev = ex->groups[group_of[j]];
    GR_EXEC_TRY(hipStreamWaitEvent(s, ev, 0));
    if (!sized) GR_EXEC_TRY(hipEventSynchronize(ev));  // the plan (pair count) sizes this view's workspaces
    const gr_plan plan = sized ? cfg->caps[j] : ex->plans[j];
    if (plan.num_pairs < 0 || plan.num_slots < 0) return gr_exec_set_error(GR_ERR_OVERFLOW, "pair count overflows int32");
    const gr_view& v = views[j].view;
    const size_t bins_bytes = gr_bins_bytes(&v, n, &plan), scratch_bytes = gr_fwd_scratch_bytes(&v, n, &plan);
    const bool ssim = op.w_dssim > 0.0f;  // the D-SSIM form (gr_fit_views_ssim)
    const size_t ws_bytes = ssim ? gr_bwd_ssim_bytes(&v, n, &plan) : gr_bwd_bytes(&v, n, &plan);
    StreamWs& W = ex->ws[k];
    GR_EXEC_TRY(W.bins.fit(bins_bytes, s));
    GR_EXEC_TRY(W.scratch.fit(scratch_bytes, s));
    if (!fwd_only) GR_EXEC_TRY(W.ws.fit(ws_bytes, s));
    void *bins = W.bins.p, *scratch = W.scratch.p, *ws = W.ws.p;
    if (fwd_only) {
      // the saved sums only (no image, no depth output), then the pass's calls on them
      GR_EXEC_TRY(W.saved.fit(gr_saved_floats(&v) * sizeof(float), s));
      GR_EXEC_TRY(W.pass.fit(pass.ws_bytes(&v, n, &plan), s));
      GR_EXEC_CALL(gr_fwd_render(&v, n, &plan, geom[j], bins, W.bins.cap, scratch, W.scratch.cap, nullptr, nullptr,
                                 nullptr, (float*)W.saved.p, s));
      GR_EXEC_CALL(pass.on_saved(j, views[j], n, &plan, geom[j], bins, W, s));
    } else if (ssim || depth) {
      // the saved-sums forms: the sums only (no image: the D-SSIM forward stages the colours from them), then the D-SSIM
      // or the depth-loss backward up to the view's sums; sums3 with a depth target
      const gr_fit_target& t = views[j];
      GR_EXEC_TRY(W.saved.fit(gr_saved_floats(&v) * sizeof(float), s));
      float* saved = (float*)W.saved.p;
      GR_EXEC_CALL(gr_fwd_render(&v, n, &plan, geom[j], bins, W.bins.cap, scratch, W.scratch.cap, nullptr, nullptr,
                                 nullptr, saved, s));
      Buf& sb = W.sums[pending[k].size()];
      Buf& s3 = W.sums3[pending[k].size()];
      GR_EXEC_TRY(sb.fit(sums_bytes, s));
      if (depth) GR_EXEC_TRY(s3.fit((size_t)n * sizeof(float), s));
      float* p3 = depth ? (float*)s3.p : nullptr;
      if (ssim)
        GR_EXEC_CALL(gr_bwd_fit_ssim_gather(&v, n, &plan, geom[j], bins, saved, t.target_rgb, t.target_mask, op.w_sil,
                                            t.target_depth, op.w_depth, op.g_scale, op.w_dssim, op.losses + j, ws, W.ws.cap,
                                            (float*)sb.p, p3, s));
      else
        GR_EXEC_CALL(gr_bwd_fit_gather(&v, n, &plan, geom[j], bins, saved, t.target_rgb, t.target_mask, op.w_sil,
                                       t.target_depth, op.w_depth, op.g_scale, op.losses + j, ws, W.ws.cap, (float*)sb.p, p3, s));
      pending[k].push_back({j, v, (float*)sb.p, p3});
    } else {
      GR_EXEC_CALL(gr_fwd_render_l1(&v, n, &plan, geom[j], bins, W.bins.cap, scratch, W.scratch.cap, views[j].target_rgb,
                                    views[j].target_mask, op.w_sil, op.g_scale, op.losses + j, nullptr, nullptr, ws,
                                    W.ws.cap, s));
      GR_EXEC_CALL(gr_bwd_splat(&v, n, &plan, geom[j], bins, ws, W.ws.cap, s));
      Buf& sb = W.sums[pending[k].size()];
      GR_EXEC_TRY(sb.fit(sums_bytes, s));
      GR_EXEC_CALL(gr_gather_view(&v, n, &plan, geom[j], bins, ws, (float*)sb.p, s));
      pending[k].push_back({j, v, (float*)sb.p, nullptr});
    }
    // the geom slot may be refilled once this stream has passed its last reader
    GeomSlot& gsl = ex->geoms[slot_of[j]];
    GR_EXEC_TRY(hipEventRecord(gsl.free_ev, s));
    gsl.pending = true;
    geom[j] = nullptr;
    GR_EXEC_CALL(prepare_upto(j + cfg->prep_ahead));
    if (!fwd_only && (int)pending[k].size() >= sizes[k].front()) {
      GR_EXEC_CALL(reduce_pending(k));
      if (sizes[k].size() > 1) sizes[k].pop_front();
    }
  }
  for (int k = 0; k < ns; ++k) GR_EXEC_CALL(reduce_pending(k));
  return GR_OK;  // the caller joins the streams (fit_views_on_device)
}
