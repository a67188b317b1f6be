// Op-program executor.  With a plan active (model_plan.hip) a forward is a straight sequence of launches: every op's launch
// record is filled from the plan's tensors and queued on the context's stream, or on a side stream for the ops of a lane.
// Also here: the two forward entry points, the debug taps that read a tensor back, and the tools that replay the program
// (per-op profile, stream / graph probe, amax collection).  The program was checked when it was loaded (model_load.hip).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "act_format.h"
#include "ta_internal.h"

static int conv_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

static const float* wptr(const ta_model* m, int64_t off) { return off < 0 ? nullptr : (const float*)(m->weights_dev + off); }

// a launch record keeps four loose ints per tensor (kernel arguments: their order stays)
static void put(const ta_strides& s, int& img, int& row, int& pix, int& off0) { img = s.img, row = s.row, pix = s.pix, off0 = s.off0; }

// tools only (TA_PROFILE_OPS=1): a HIP event pair around every op, then one table per forward on stderr
static void print_op_profile(ta_model* m, std::vector<hipEvent_t>& ev) {
  (void)hipStreamSynchronize(m->ctx->stream);
  double tot_ms = 0, tot_fl = 0;
  for (size_t oi = 0; oi < m->ops.size(); ++oi) {
    const ta_op_desc& op = m->ops[oi];
    const ta_tensor& to = m->tensor(op.out);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev[2 * oi], ev[2 * oi + 1]);
    const ta_tensor& ti = m->tensor(op.in);
    // a conv with a fused 2x2 max-pool computes every pixel of the UNPOOLED map: count those, not the pooled output
    const double M = op.type == TA_OP_CONV && op.pool
                         ? (double)m->run_n * conv_out(ti.h, op.kh, op.stride, op.pad) * conv_out(ti.w, op.kw, op.stride, op.pad)
                         : (double)m->run_n * to.h * to.w;
    const double fl = (op.type == TA_OP_CONV || op.type == TA_OP_DWPW) ? 2.0 * op.macs_per_pixel * M : 0.0;
    tot_ms += ms;
    tot_fl += fl;
    fprintf(stderr, "op %3zu type %d k%dx%d s%d g%d cin %4d cout %4d  %3dx%-3d M %8.0f slabs %4d  %8.1f us %7.1f TF\n", oi, op.type, op.kh,
            op.kw, op.stride, op.groups, op.cin, op.cout, to.h, to.w, M, op.n_slabs, ms * 1e3, ms > 0 ? fl / (ms * 1e-3) / 1e12 : 0.0);
  }
  fprintf(stderr, "model kind %d n %d: %.3f ms in ops, %.1f GFLOP, %.1f TF\n", m->kind, m->run_n, tot_ms, tot_fl / 1e9, tot_fl / (tot_ms * 1e-3) / 1e12);
  for (auto e : ev) (void)hipEventDestroy(e);
}

int ta_model_run_ops(ta_model* m) {
  ta_ctx* ctx = m->ctx;
  static const bool prof_ops = getenv("TA_PROFILE_OPS") != nullptr;
  std::vector<hipEvent_t> ev;
  if (prof_ops) {
    ev.resize(2 * m->ops.size());
    for (auto& e : ev) (void)hipEventCreate(&e);
  }
  struct fin_t {
    ta_model* m;
    std::vector<hipEvent_t>& ev;
    bool on;
    ~fin_t() { if (on) print_op_profile(m, ev); }
  } fin{m, ev, prof_ops};
  // lanes: an op with lane L != 0 goes to side stream L - 1, which first waits for everything queued on the main stream
  // so far (the packer places a branch right behind the op that produces its input); the main stream waits for the
  // branches at the end of the program.  The loader checked that nothing outside a branch touches what it writes.
  const bool lanes_on = !prof_ops && !ctx->profiling;                     // profiles time a serial program
  struct lanes_t {
    ta_ctx* ctx;
    hipStream_t main;
    bool started[2] = {false, false};
    ~lanes_t() {                                                           // also on an error return
      ctx->stream = main;
      for (int i = 0; i < 2; ++i)
        if (started[i]) {
          (void)hipEventRecord(ctx->side_join[i], ctx->side_stream[i]);
          (void)hipStreamWaitEvent(main, ctx->side_join[i], 0);
        }
    }
  } lanes{ctx, ctx->stream};
  const ta_plan& pl = *m->active;
  for (size_t oi = 0; oi < m->ops.size(); ++oi) {
    const ta_op_desc& op = m->ops[oi];
    const ta_tensor& ti = m->tensor(op.in);
    const ta_tensor& to = m->tensor(op.out);
    const int lane = lanes_on ? ta_op_lane(op) : 0;
    ctx->stream = lanes.main;
    if (lane) {
      const int li = lane - 1;
      if (!ctx->side_stream[li]) {
        TA_HIP(ctx, hipStreamCreateWithFlags(&ctx->side_stream[li], hipStreamNonBlocking));
        TA_HIP(ctx, hipEventCreateWithFlags(&ctx->side_fork[li], hipEventDisableTiming));
        TA_HIP(ctx, hipEventCreateWithFlags(&ctx->side_join[li], hipEventDisableTiming));
      }
      if (!lanes.started[li]) {
        TA_HIP(ctx, hipEventRecord(ctx->side_fork[li], lanes.main));
        TA_HIP(ctx, hipStreamWaitEvent(ctx->side_stream[li], ctx->side_fork[li], 0));
        lanes.started[li] = true;
      }
      ctx->stream = ctx->side_stream[li];
    }
    struct evp_t {
      hipEvent_t e;
      hipStream_t s;
      bool on;
      ~evp_t() { if (on) (void)hipEventRecord(e, s); }
    } evp{prof_ops ? ev[2 * oi + 1] : nullptr, ctx->stream, prof_ops};
    if (prof_ops) (void)hipEventRecord(ev[2 * oi], ctx->stream);
    switch (op.type) {
      case TA_OP_CONV: {
        ta_conv_launch p;
        memset(&p, 0, sizeof(p));
        p.in = ti.dev;
        p.w = wptr(m, op.w_off);
        p.ktab = pl.ktab_dev + pl.ktab_off[oi];
        p.bias = wptr(m, op.bias_off);
        p.prelu = wptr(m, op.prelu_off);
        p.out = to.dev;
        p.M = m->run_n * to.h * to.w;
        p.Ho = to.h;
        p.Wo = to.w;
        p.n_slabs = op.n_slabs;
        p.coutp = op.coutp;
        p.cout = op.cout;
        p.act = op.act;
        p.stride = op.stride;
        p.prec = op.prec;
        const ta_k_geometry kg = ta_conv_k_geometry(op, ti.fmt);
        p.uniform_k = kg.uniform;
        p.k_cblocks = kg.cblocks;
        p.k_w = op.kw;
        p.k_h = op.kh;
        p.in_ch_off = op.in_ch_off;
        put(ta_tensor_strides(ti, op.pad, false), p.in_img, p.in_row, p.in_pix, p.in_off0);
        p.win_wp = ti.wp();
        p.win_img = ti.hp() * ti.wp();
        put(ta_tensor_strides(to, 0, false), p.out_img, p.out_row, p.out_pix, p.out_off0);
        p.out_ch = op.out_ch_off;
        p.out_fmt = to.fmt;
        p.in_fmt = ti.fmt;
        if (op.res >= 0) {
          const ta_tensor& tr = m->tensor(op.res);
          p.res = tr.dev;
          put(ta_tensor_strides(tr, 0, false), p.res_img, p.res_row, p.res_pix, p.res_off0);
          p.res_ch = op.res_ch_off;
          p.res_fmt = tr.fmt;
          p.res_up2 = op.res_up2;
        }
        if (op.out2 >= 0) {
          const ta_tensor& t2 = m->tensor(op.out2);
          p.out2 = t2.dev;
          p.scale2 = wptr(m, op.scale2_off);
          p.shift2 = wptr(m, op.shift2_off);
          put(ta_tensor_strides(t2, 0, false), p.o2_img, p.o2_row, p.o2_pix, p.o2_off0);
          p.o2_ch = op.out2_ch_off;
          p.o2_fmt = t2.fmt;
        }
        if (op.groups > 1) {
          p.group_cout = op.cout / op.groups;
          p.group_cin = op.cin;
        }
        p.variant = ta_op_forced_variant(op);
        if (ta_op_border_bias(op)) p.bias9 = wptr(m, op.scale2_off);
        // a tensor no op reads is a float32 RESULT (embeddings, detector heads): nothing splits it into half floats, whatever it holds
        p.range_check = (m->has_half_ops && (m->tensor_read[op.out] || (op.out2 >= 0 && m->tensor_read[op.out2]))) ? 1 : 0;
        p.amax_index = (m->amax_on && oi < TA_AMAX_OPS) ? (int)oi : -1;
        double flops = 2.0 * op.macs_per_pixel * (double)p.M;
        if (op.pool) {
          p.pool = 1;
          p.M = m->run_n * to.h * to.w * 4;            // the four pixels of every 2x2 window
          flops = 2.0 * op.macs_per_pixel * (double)m->run_n * conv_out(ti.h, op.kh, op.stride, op.pad) *
                  conv_out(ti.w, op.kw, op.stride, op.pad);   // algorithmic: the whole conv output, odd edge included
        }
        p.k_split = pl.splitk_ws ? ta_op_ksplit(op, ti.fmt) : 1;
        p.partial = pl.splitk_ws;
        if (lane) p.k_split = 1;                       // the K-split workspace belongs to the main stream
        TA_TRY(ta_launch_conv(ctx, p, flops));
        break;
      }
      case TA_OP_RFSTEM:
        TA_TRY(ta_launch_rfstem(ctx, m->input_u8, m->run_n, ti.h, ti.w, (const float*)m->weights_host_small.data(),
                                op.cout == 32 ? wptr(m, op.w_off) + 448 : nullptr, to));
        break;
      case TA_OP_DWPW: {
        ta_conv_launch p;
        memset(&p, 0, sizeof(p));
        p.in = ti.dev;
        p.w = wptr(m, op.w_off);
        p.bias = wptr(m, op.bias_off);
        p.dw_w = wptr(m, op.scale2_off);          // [9][cin]   (the op reuses the second-output fields for the depthwise part)
        p.dw_bias = wptr(m, op.shift2_off);       // [cin]
        p.dw_c = op.cin;
        p.dw_stride = op.stride;
        p.out = to.dev;
        p.M = m->run_n * to.h * to.w;
        p.Ho = to.h;
        p.Wo = to.w;
        p.n_slabs = op.n_slabs;
        p.coutp = op.coutp;
        p.cout = op.cout;
        p.act = op.act;
        p.stride = 1;
        p.prec = op.prec;
        p.range_check = (m->has_half_ops && m->tensor_read[op.out]) ? 1 : 0;
        p.amax_index = (m->amax_on && oi < TA_AMAX_OPS) ? (int)oi : -1;
        put(ta_tensor_strides(ti, 1, true), p.in_img, p.in_row, p.in_pix, p.in_off0);
        p.in_fmt = ti.fmt;
        put(ta_tensor_strides(to, 0, true), p.out_img, p.out_row, p.out_pix, p.out_off0);
        p.out_ch = op.out_ch_off;
        p.out_fmt = to.fmt;
        TA_TRY(ta_launch_dwpw(ctx, p, 2.0 * op.macs_per_pixel * (double)p.M));
        break;
      }
      case TA_OP_DWCONV: {
        ta_dw_launch p;
        memset(&p, 0, sizeof(p));
        p.in = ti.dev;
        p.w = wptr(m, op.w_off);
        p.bias = wptr(m, op.bias_off);
        p.out = to.dev;
        p.N = m->run_n;
        p.Ho = to.h;
        p.Wo = to.w;
        p.C = op.cin;
        p.stride = op.stride;
        p.relu = op.act == TA_ACT_RELU;
        put(ta_tensor_strides(ti, op.pad, true), p.in_img, p.in_row, p.in_pix, p.in_off0);
        p.in_fmt = ti.fmt;
        put(ta_tensor_strides(to, 0, true), p.out_img, p.out_row, p.out_pix, p.out_off0);
        p.out_fmt = to.fmt;
        TA_TRY(ta_launch_dwconv(ctx, p));
        break;
      }
      case TA_OP_MAXPOOL:
        TA_TRY(ta_launch_maxpool(ctx, ti, to, m->run_n));
        break;
      case TA_OP_COPYCH:
        TA_TRY(ta_launch_copych(ctx, ti, op.in_ch_off, to, op.out_ch_off, op.cin, m->run_n));
        break;
    }
  }
  return TA_OK;
}

extern "C" {

// tools (tools/graph_probe.py): the op program of the LAST forward (same plan, same input) replayed `reps` times as plain stream
// launches and as a hipGraph captured from them (lanes = fork / join through events: part of the capture).
// out_ms[0] / [1]: GPU time per replay, streams / graph (HIP events on the main stream); out_ms[2] / [3]: host time the
// enqueue of one replay takes, streams / graph; out_ms[4]: capture + instantiate, once.
int ta_model_graph_probe(ta_model* m, int reps, double* out_ms) {
  ta_enter(m ? m->ctx : nullptr);
  if (!m || !out_ms || reps < 1) return TA_E_INVALID;
  ta_ctx* ctx = m->ctx;
  if (!m->active) return ta_fail(ctx, TA_E_INVALID, "graph_probe: run a forward first (it replays that plan)");
  struct res_t {                                      // released on every return path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~res_t() {
      if (exec) (void)hipGraphExecDestroy(exec);
      if (graph) (void)hipGraphDestroy(graph);
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } r;
  hipEvent_t& e0 = r.e0;
  hipEvent_t& e1 = r.e1;
  hipGraph_t& graph = r.graph;
  hipGraphExec_t& exec = r.exec;
  TA_HIP(ctx, hipEventCreate(&e0));
  TA_HIP(ctx, hipEventCreate(&e1));
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  for (int i = 0; i < 2; ++i) TA_TRY(ta_model_run_ops(m));          // lazy state (function attributes, side streams) exists
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  double t0 = now();
  TA_HIP(ctx, hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < reps; ++i) TA_TRY(ta_model_run_ops(m));
  TA_HIP(ctx, hipEventRecord(e1, ctx->stream));
  out_ms[2] = (now() - t0) / reps;
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TA_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
  out_ms[0] = ms / reps;
  t0 = now();
  TA_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
  const int rc = ta_model_run_ops(m);
  const hipError_t ce = hipStreamEndCapture(ctx->stream, &graph);
  if (rc != TA_OK) return rc;
  TA_HIP(ctx, ce);
  TA_HIP(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  out_ms[4] = now() - t0;
  for (int i = 0; i < 2; ++i) TA_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  t0 = now();
  TA_HIP(ctx, hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < reps; ++i) TA_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
  TA_HIP(ctx, hipEventRecord(e1, ctx->stream));
  out_ms[3] = (now() - t0) / reps;
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TA_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
  out_ms[1] = ms / reps;
  return TA_OK;
}

int ta_model_debug_amax(ta_model* m, int enable, float* out, int capacity) {
  ta_enter(m ? m->ctx : nullptr);
  if (!m) return TA_E_INVALID;
  ta_ctx* ctx = m->ctx;
  const size_t n = 2 * std::min(m->ops.size(), (size_t)TA_AMAX_OPS);
  unsigned* slots = (unsigned*)ctx->range_flag + TA_AMAX_SLOT0;      // one set per context: one model collects at a time
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (out) {
    if (!m->amax_on) return ta_fail(ctx, TA_E_INVALID, "debug_amax: not enabled");
    if ((size_t)capacity < 2 * m->ops.size()) return ta_fail(ctx, TA_E_CAPACITY, "debug_amax: %zu floats needed", 2 * m->ops.size());
    memset(out, 0, 2 * m->ops.size() * sizeof(float));
    TA_HIP(ctx, hipMemcpy(out, slots, n * sizeof(float), hipMemcpyDeviceToHost));   // bit patterns of |x| ARE the floats
  }
  if (enable == 2) return TA_OK;                 // read only: the collection goes on
  if (enable) {
    // the slots belong to the context, the switch to the model: a second model of the same context must not zero or overwrite
    // what the first one is collecting
    if (ctx->amax_owner && ctx->amax_owner != m)
      return ta_fail(ctx, TA_E_INVALID, "debug_amax: another model of this context is collecting (disable it first)");
    TA_HIP(ctx, hipMemset(slots, 0, 2 * TA_AMAX_OPS * sizeof(unsigned)));
    ctx->amax_owner = m;
  } else if (ctx->amax_owner == m) {
    ctx->amax_owner = nullptr;
  }
  m->amax_on = enable != 0;
  return TA_OK;
}

int ta_model_forward_frames(ta_model* m, const ta_frames* f) {
  ta_enter(m ? m->ctx : nullptr);
  if (!m || !f) return TA_E_INVALID;
  ta_ctx* ctx = m->ctx;
  if (m->kind != TA_MODEL_RETINAFACE && m->kind != TA_MODEL_OPENPOSE)
    return ta_fail(ctx, TA_E_INVALID, "forward_frames: model kind %d takes crops", m->kind);
  if (f->n == 0) return TA_OK;
  TA_TRY(ta_model_plan(m, f->n, f->h, f->w));
  m->input_u8 = f->dev;
  if (m->ops[0].type != TA_OP_RFSTEM)              // that op reads the frames itself
    TA_TRY(ta_launch_preprocess(ctx, m->kind == TA_MODEL_RETINAFACE ? TA_PRE_RETINAFACE : TA_PRE_OPENPOSE, f->dev, f->n,
                                f->h, f->w, m->tensor(m->hdr.input_tensor)));
  return ta_model_run_ops(m);
}

int ta_model_forward_crops(ta_model* m, const uint8_t* crops, int n) {
  ta_enter(m ? m->ctx : nullptr);
  if (!m || (!crops && n > 0)) return TA_E_INVALID;
  ta_ctx* ctx = m->ctx;
  if (m->kind != TA_MODEL_ARCFACE) return ta_fail(ctx, TA_E_INVALID, "forward_crops: not an ArcFace model");
  if (n == 0) return TA_OK;
  TA_TRY(ta_model_plan(m, n, 112, 112));
  void* scr = nullptr;
  const size_t bytes = (size_t)n * 3 * 112 * 112;
  TA_TRY(ta_scratch(ctx, bytes, &scr));
  TA_HIP(ctx, hipMemcpyAsync(scr, crops, bytes, hipMemcpyHostToDevice, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TA_TRY(ta_launch_preprocess(ctx, TA_PRE_ARCFACE_CROPS, (const uint8_t*)scr, n, 112, 112,
                              m->tensor(m->hdr.input_tensor)));
  return ta_model_run_ops(m);
}

int ta_model_tensor_shape(ta_model* m, int tensor, int* n, int* c, int* h, int* w) {
  if (!m || !m->active || tensor < 0 || tensor >= m->hdr.n_tensors) return TA_E_INVALID;
  const ta_tensor& t = m->tensor(tensor);
  if (n) *n = m->run_n;
  if (c) *c = t.c;
  if (h) *h = t.h;
  if (w) *w = t.w;
  return TA_OK;
}

int ta_model_read_tensor(ta_model* m, int tensor, int ch_off, int ch, float* dst) {
  ta_enter(m ? m->ctx : nullptr);
  if (!m || !dst || !m->active || tensor < 0 || tensor >= m->hdr.n_tensors) return TA_E_INVALID;
  ta_ctx* ctx = m->ctx;
  const ta_tensor& t = m->tensor(tensor);
  if (!t.dev || ch_off < 0 || ch <= 0 || ch_off + ch > t.c) return ta_fail(ctx, TA_E_INVALID, "read_tensor: bad slice");
  std::vector<float> host((size_t)m->run_n * t.hp() * t.wp() * t.c);
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TA_HIP(ctx, hipMemcpy(host.data(), t.dev, host.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < m->run_n; ++i)
    for (int c = 0; c < ch; ++c)
      for (int y = 0; y < t.h; ++y)
        for (int x = 0; x < t.w; ++x)
        {
          const int cc = ch_off + c;
          float v;
          if (t.fmt == TA_FMT_F16) {
            _Float16 hh;
            memcpy(&hh, (const char*)&host[t.off(i, y, x)] + 2 * cc, 2);
            v = (float)hh;
          } else if (t.fmt != TA_FMT_F32) {
            const char* b = (const char*)&host[t.off(i, y, x)] + ((cc >> 5) << 7) + ((cc & 31) << 1);
            uint16_t h16, l16;
            memcpy(&h16, b, 2);
            memcpy(&l16, b + 64, 2);
            if (t.fmt == TA_FMT_SPLIT16) {
              _Float16 hh, ll;
              memcpy(&hh, &h16, 2);
              memcpy(&ll, &l16, 2);
              v = (float)hh + (float)ll;
            } else {
              const uint32_t hb = (uint32_t)h16 << 16, lb = (uint32_t)l16 << 16;
              float hf, lf;
              memcpy(&hf, &hb, 4);
              memcpy(&lf, &lb, 4);
              v = hf + lf;
            }
          } else {
            v = host[t.off(i, y, x) + cc];
          }
          dst[(((size_t)i * ch + c) * t.h + y) * t.w + x] = t.unscale_host ? v * t.unscale_host[cc] : v;   // channel cc is stored times 2^a[cc]
        }
  return TA_OK;
}

}  // extern "C"
