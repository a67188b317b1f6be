// Per-shape activation planner.  A plan is everything about a loaded model that depends on the input shape (N, H, W): every
// tensor's spatial size, one zero-filled HBM arena that holds all of them side by side (no buffer reuse: the zero halos must
// stay intact) with the K-split workspace behind them, and the K-offset tables of the table-driven convs.  A model keeps a
// small LRU of plans.  The program was checked when it was loaded (model_load.hip): planning fails only on what depends on
// the shape -- an input too small for the network, a tensor written with two sizes, a view that does not match its source,
// a tensor over 4 GiB -- and on the device.
#include <algorithm>

#include "act_format.h"
#include "ta_internal.h"

#define TA_MAX_PLANS 4
#define TA_MAX_PLAN_BYTES ((size_t)96 << 30)

static int conv_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

static void activate(ta_model* m, ta_plan* pl, int n_run) {
  m->active = pl;
  pl->last_use = ++m->use_counter;
  m->run_n = n_run;
}

// Batch capacity a plan is carved for.  Frame batches (RetinaFace / OpenPose) come in a few fixed sizes; the ArcFace
// batch is the number of faces in a frame batch and changes on almost every call of a video loop, so its plans are
// carved for a bucketed capacity (8, 32, then multiples of 64) and reused for every smaller count: no stream sync,
// hipMalloc / memset of a multi-GB arena or eviction hipFree per distinct face count.  Launches always cover exactly
// the n crops of the call (ta_model::run_n); the unused tail of the arena is never touched.
static int plan_capacity(int kind, int n) {
  if (kind != TA_MODEL_ARCFACE) return n;
  if (n <= 8) return 8;
  if (n <= 32) return 32;
  return (n + 63) / 64 * 64;
}

// Sizes of every tensor for an h x w input, by walking the program once.
static int infer_shapes(const ta_model* m, int h, int w, std::vector<ta_tensor>& ts, std::vector<bool>& set) {
  ta_ctx* ctx = m->ctx;
  ts[m->hdr.input_tensor].h = h;
  ts[m->hdr.input_tensor].w = w;
  set[m->hdr.input_tensor] = true;

  auto resolve_alias = [&](int id) -> int {
    const int src = m->tdesc[id].alias_of;
    if (src == -2) ts[id].owns = false;            // shape only
    if (src < 0 || set[id]) return TA_OK;
    if (ts[src].halo != 0 || (size_t)ts[src].h * ts[src].w * ts[src].c != (size_t)ts[id].c)
      return ta_fail(ctx, TA_E_INVALID, "plan: alias tensor %d does not match source %d", id, src);
    ts[id].h = ts[id].w = 1;
    ts[id].owns = false;
    set[id] = true;
    return TA_OK;
  };
  auto set_out = [&](int id, int oh, int ow) -> int {
    if (oh <= 0 || ow <= 0) return ta_fail(ctx, TA_E_INVALID, "plan: input %dx%d too small for the network", h, w);
    if (set[id] && (ts[id].h != oh || ts[id].w != ow))
      return ta_fail(ctx, TA_E_INVALID, "plan: tensor %d written with %dx%d and %dx%d", id, ts[id].h, ts[id].w, oh, ow);
    ts[id].h = oh;
    ts[id].w = ow;
    set[id] = true;
    return TA_OK;
  };

  for (const ta_op_desc& op : m->ops) {
    TA_TRY(resolve_alias(op.in));
    const ta_tensor& ti = ts[op.in];
    switch (op.type) {
      case TA_OP_CONV:
      case TA_OP_DWCONV: {
        const int oh = conv_out(ti.h, op.kh, op.stride, op.pad), ow = conv_out(ti.w, op.kw, op.stride, op.pad);
        if (op.type == TA_OP_CONV && op.pool) {      // 2x2 / 2 max-pool (floor) in the conv's epilogue
          TA_TRY(set_out(op.out, oh / 2, ow / 2));
          break;
        }
        TA_TRY(set_out(op.out, oh, ow));
        if (op.type == TA_OP_CONV && op.out2 >= 0) TA_TRY(set_out(op.out2, oh, ow));
        break;
      }
      case TA_OP_MAXPOOL:
        TA_TRY(set_out(op.out, ti.h / 2, ti.w / 2));
        break;
      case TA_OP_RFSTEM:
        if (op.cout == 32)                           // fused with the next block (dw3x3 s2 -> 1x1 16 -> 32): quarter resolution
          TA_TRY(set_out(op.out, ((ti.h + 1) / 2 + 1) / 2, ((ti.w + 1) / 2 + 1) / 2));
        else
          TA_TRY(set_out(op.out, (ti.h + 1) / 2, (ti.w + 1) / 2));
        break;
      case TA_OP_DWPW:
        TA_TRY(set_out(op.out, conv_out(ti.h, 3, op.stride, 1), conv_out(ti.w, 3, op.stride, 1)));
        break;
      case TA_OP_COPYCH:
        TA_TRY(set_out(op.out, ti.h, ti.w));
        break;
    }
  }
  for (size_t i = 0; i < ts.size(); ++i) TA_TRY(resolve_alias((int)i));
  return TA_OK;
}

int ta_model_plan(ta_model* m, int n_run, int h, int w) {
  ta_ctx* ctx = m->ctx;
  if (n_run <= 0 || h <= 0 || w <= 0) return ta_fail(ctx, TA_E_INVALID, "plan: bad input shape %dx%dx%d", n_run, h, w);
  const int n = plan_capacity(m->kind, n_run);
  auto fits = [&](const ta_plan* pl) { return pl && pl->n == n && pl->h == h && pl->w == w; };
  if (fits(m->active)) {
    activate(m, m->active, n_run);
    return TA_OK;
  }
  for (auto& pl : m->plans)
    if (fits(pl.get())) {
      activate(m, pl.get(), n_run);
      return TA_OK;
    }
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // evict least-recently-used plans beyond the count / byte budget
  for (;;) {
    size_t bytes = 0;
    for (auto& pl : m->plans) bytes += pl->arena_bytes;
    if (m->plans.size() < TA_MAX_PLANS && bytes <= TA_MAX_PLAN_BYTES) break;
    if (m->plans.empty()) break;
    size_t lru = 0;
    for (size_t i = 1; i < m->plans.size(); ++i)
      if (m->plans[i]->last_use < m->plans[lru]->last_use) lru = i;
    if (m->plans[lru].get() == m->active) m->active = nullptr;
    m->plans.erase(m->plans.begin() + lru);
  }
  std::unique_ptr<ta_plan> np(new ta_plan());        // freed with its device memory on every failure below
  np->n = n;
  np->h = h;
  np->w = w;

  const int T = m->hdr.n_tensors;
  std::vector<ta_tensor> ts(T);
  std::vector<bool> set(T, false);
  for (int i = 0; i < T; ++i) {
    ts[i].c = m->tdesc[i].channels;
    ts[i].halo = m->tdesc[i].halo;
    ts[i].fmt = m->tdesc[i].fmt;
    if (m->tdesc[i].unscale_off >= 0) {
      ts[i].unscale_dev = (const float*)(m->weights_dev + m->tdesc[i].unscale_off);
      ts[i].unscale_host = m->unscale_host[i].data();
    }
    ts[i].n = n;
  }
  TA_TRY(infer_shapes(m, h, w, ts, set));

  // carve the arena
  size_t total = 0;
  std::vector<size_t> offs(T, 0);
  for (int i = 0; i < T; ++i) {
    if (!set[i] || !ts[i].owns) continue;
    const size_t bytes = ts[i].elems() * sizeof(float);
    if (bytes >= ((size_t)1 << 32)) return ta_fail(ctx, TA_E_INVALID, "plan: tensor %d exceeds 4 GiB; split the batch", i);
    offs[i] = total;
    total += (bytes + 255) & ~(size_t)255;
  }
  // workspace of the K-split convs (see ta_conv_ksplit): the largest partial[k][pixel][coutp] any op needs
  size_t ws_bytes = 0;
  for (const ta_op_desc& op : m->ops) {
    if (op.type != TA_OP_CONV) continue;
    const int M = ts[op.out].n * ts[op.out].h * ts[op.out].w;
    const int ks = ta_op_ksplit(op, ts[op.in].fmt);
    if (ks > 1) ws_bytes = std::max(ws_bytes, (size_t)ks * M * op.coutp * sizeof(float));
  }
  const size_t ws_off = total;
  total += (ws_bytes + 255) & ~(size_t)255;
  hipError_t e = hipMalloc((void**)&np->arena, total ? total : 256);
  if (e != hipSuccess) {
    np->arena = nullptr;
    return ta_fail(ctx, TA_E_DEVICE, "plan: hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
  }
  np->arena_bytes = total;
  TA_HIP(ctx, hipMemsetAsync(np->arena, 0, total ? total : 256, ctx->stream));
  for (int i = 0; i < T; ++i)
    if (set[i] && ts[i].owns) ts[i].dev = (float*)(np->arena + offs[i]);
  for (int i = 0; i < T; ++i)
    if (set[i] && !ts[i].owns) ts[i].dev = m->tdesc[i].alias_of >= 0 ? ts[m->tdesc[i].alias_of].dev : nullptr;
  np->splitk_ws = ws_bytes ? (float*)(np->arena + ws_off) : nullptr;

  // K-offset tables: 8 entries (4 channels each) per slab of a conv that does not read a half-float tensor (those run on
  // the split-role kernels only: uniform K walk, no table)
  std::vector<int32_t> ktab;
  np->ktab_off.assign(m->ops.size(), 0);
  for (size_t oi = 0; oi < m->ops.size(); ++oi) {
    const ta_op_desc& op = m->ops[oi];
    if (op.type != TA_OP_CONV) continue;
    const ta_tensor& ti = ts[op.in];
    np->ktab_off[oi] = ktab.size();
    if (ti.fmt == TA_FMT_F16) continue;
    const int cpt = op.cin / 4;
    const int nq = op.kh * op.kw * cpt;
    for (int q = 0; q < op.n_slabs * 8; ++q) {
      int32_t off = 0;
      if (q < nq) {
        const int tap = q / cpt, ch = (q % cpt) * 4;
        const int ky = tap / op.kw, kx = tap % op.kw;
        off = (int32_t)((((size_t)ky * ti.wp() + kx) * ti.c + op.in_ch_off + ch) * sizeof(float));
      }
      ktab.push_back(off);
    }
  }
  if (!ktab.empty()) {
    TA_HIP(ctx, hipMalloc((void**)&np->ktab_dev, ktab.size() * sizeof(int32_t)));
    TA_HIP(ctx, hipMemcpy(np->ktab_dev, ktab.data(), ktab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  np->tensors.swap(ts);
  m->plans.push_back(std::move(np));
  activate(m, m->plans.back().get(), n_run);
  return TA_OK;
}
