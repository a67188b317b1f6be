// Packed-model loader.  A blob (terran_amd/pack/: header, tensor table, op table, weight region) is parsed into host structs
// and refused here, once, if anything that depends on the program alone is wrong (ta_program_parse / ta_program_check: no
// context, no HIP call); ta_model_load then uploads the weight region.  Shapes, arenas and launches are the planner's and
// the executor's (model_plan.hip, model_run.hip), which may assume a checked program.
#include <stdarg.h>
#include <string.h>

#include "act_format.h"
#include "ta_internal.h"

namespace {
struct refusal {                       // writes the defect into the caller's buffer
  char* msg;
  size_t cap;
  int operator()(const char* fmt, ...) const {
    if (msg && cap) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(msg, cap, fmt, ap);
      va_end(ap);
    }
    return TA_E_INVALID;
  }
};
const int MAX_DIM = 1 << 24;           // channel counts, channel offsets, K slabs: every product below stays inside int64
bool within(int v, int lo, int hi) { return v >= lo && v <= hi; }
}  // namespace

int ta_program_parse(int kind, const void* blob, size_t bytes, ta_program* out, char* msg, size_t msg_capacity) {
  const refusal no{msg, msg_capacity};
  if (msg && msg_capacity) msg[0] = 0;
  if (!blob || !out) return no("model blob: null pointer");
  if (bytes < sizeof(ta_blob_header)) return no("model blob too small");
  ta_blob_header& h = out->hdr;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != TA_BLOB_MAGIC || h.version != 9) return no("model blob: bad magic/version (this library reads version 9)");
  if (h.kind != kind) return no("model blob is kind %d, expected %d", h.kind, kind);
  if (h.n_tensors <= 0 || h.n_ops <= 0 || h.n_outputs < 0 || h.n_outputs > 16 || h.input_tensor < 0 ||
      h.input_tensor >= h.n_tensors)
    return no("model blob: bad counts");
  auto inside = [&](int64_t off, int64_t count, size_t each) {
    return off >= 0 && count >= 0 && (uint64_t)off <= bytes && (uint64_t)count <= (bytes - (size_t)off) / each;
  };
  if (!inside(h.tensors_off, h.n_tensors, sizeof(ta_tensor_desc))) return no("model blob: truncated (tensor table)");
  if (!inside(h.ops_off, h.n_ops, sizeof(ta_op_desc))) return no("model blob: truncated (op table)");
  if (!inside(h.weights_off, h.weights_bytes, 1)) return no("model blob: truncated (weights)");
  const int T = h.n_tensors;
  std::vector<ta_tensor_desc>& td = out->tdesc;
  std::vector<ta_op_desc>& ops = out->ops;
  td.resize(T);
  ops.resize(h.n_ops);
  memcpy(td.data(), (const char*)blob + h.tensors_off, T * sizeof(ta_tensor_desc));
  memcpy(ops.data(), (const char*)blob + h.ops_off, h.n_ops * sizeof(ta_op_desc));
  auto bad_w = [&](int64_t off, size_t need) { return off >= 0 && (uint64_t)off + need > (uint64_t)h.weights_bytes; };

  for (int t = 0; t < T; ++t) {
    const ta_tensor_desc& d = td[t];
    if (!within(d.channels, 1, MAX_DIM) || !within(d.halo, 0, 1024) || !within(d.alias_of, -2, T - 1) || d.alias_of == t)
      return no("model blob: malformed tensor %d", t);
    if ((d.fmt != TA_FMT_F32 && d.channels % 32) || (d.fmt == TA_FMT_F16 && d.channels % 64) || d.fmt < 0 || d.fmt > TA_FMT_F16)
      return no("model blob: tensor %d: format %d with %d channels", t, d.fmt, d.channels);
    // activation scales: an optional vector of per-channel powers of two in the weights region; the input is read by the
    // pre-processing kernels as it is
    if (d.unscale_off >= 0 && (t == h.input_tensor || (d.unscale_off & 3) || bad_w(d.unscale_off, (size_t)d.channels * sizeof(float))))
      return no("model blob: inconsistent activation scales (tensor %d)", t);
  }
  for (int i = 0; i < h.n_outputs; ++i)
    if (!within(h.outputs[i], 0, T - 1)) return no("model blob: output %d is tensor %d, out of range", i, h.outputs[i]);

  // tensors that have a size when an op reads them: the input, what earlier ops wrote, views of those
  std::vector<char> set(T, 0);
  set[h.input_tensor] = 1;
  auto view_ready = [&](int id) {
    const int src = td[id].alias_of;
    if (src >= 0 && !set[id]) set[id] = set[src];
    return src < 0 || set[id];
  };
  // lanes: a branch may read what earlier main-stream ops wrote and its own tensors; nothing outside the branch may touch
  // what it writes, nothing later may write what it reads, and it takes plain convs only
  std::vector<int> writer_lane(T, 0), reader_lanes(T, 0);

  for (int oi = 0; oi < h.n_ops; ++oi) {
    const ta_op_desc& op = ops[oi];
    auto bad_t = [&](int t) { return t < 0 || t >= T; };
    const char* why = nullptr;                                   // the first defect of the record
    auto need = [&](bool ok, const char* what) {
      if (!ok && !why) why = what;
    };
    need(!bad_t(op.in) && !bad_t(op.out) && (op.res < 0 || !bad_t(op.res)) && (op.out2 < 0 || !bad_t(op.out2)), "tensor index out of range");
    need(within(op.kh, 1, 64) && within(op.kw, 1, 64) && within(op.stride, 1, 64) && within(op.pad, 0, 64) && within(op.cin, 0, MAX_DIM) &&
             within(op.cout, 0, MAX_DIM) && within(op.coutp, 0, MAX_DIM) && within(op.n_slabs, 0, MAX_DIM) && within(op.groups, 0, 1 << 16) &&
             within(op.in_ch_off, 0, MAX_DIM) && within(op.out_ch_off, 0, MAX_DIM) && within(op.res_ch_off, 0, MAX_DIM) &&
             within(op.out2_ch_off, 0, MAX_DIM),
         "field out of range");
    if (why) return no("model blob: malformed op %d: %s", oi, why);
    const size_t row = (size_t)op.coutp * 4, image = (size_t)op.n_slabs * op.coutp * 128;
    const bool wus_ok = !bad_w(op.bias_off, row) && op.wus_off == op.bias_off + 4 * (int64_t)op.coutp && !bad_w(op.wus_off, row);
    if (op.type == TA_OP_CONV) {
      need(op.w_off >= 0 && op.bias_off >= 0, "no weights or no bias");
      need(op.cin % 4 == 0 && op.cout % 4 == 0 && op.coutp % 32 == 0 && op.n_slabs > 0, "channel counts or K slabs");
      need(op.prec >= 0 && op.prec <= 5, "arithmetic mode");
      need(!bad_w(op.w_off, image), "w_off past the weight region");
      need(!bad_w(op.bias_off, row), "bias_off past the weight region");
      need(!bad_w(op.prelu_off, row), "prelu_off past the weight region");
      need(!bad_w(op.scale2_off, row), "scale2_off past the weight region");
      need(!bad_w(op.shift2_off, row), "shift2_off past the weight region");
      need(wus_ok, "wus_off is not the [coutp] floats behind the bias");
      need(op.act != TA_ACT_PRELU || op.prelu_off >= 0, "PReLU without slopes");
      need(op.out2 < 0 || (op.scale2_off >= 0 && op.shift2_off >= 0), "second output without its affine");
      need(!ta_op_border_bias(op) || !(op.out2 >= 0 || op.scale2_off < 0 || op.kh != 3 || op.kw != 3 || op.stride != 1 || op.pad != 1 ||
                                       op.pool || bad_w(op.scale2_off, 16 * row)),
           "border-bias table on a conv that is not a plain 3x3, stride 1, pad 1");
    } else if (op.type == TA_OP_RFSTEM) {
      need(op.w_off >= 0 && (op.cout == 16 || op.cout == 32), "front op without weights or with another width than 16 / 32");
      need(!bad_w(op.w_off, (op.cout == 32 ? 448 + 704 : 448) * 4), "w_off past the weight region");
    } else if (op.type == TA_OP_DWPW) {
      need(op.w_off >= 0 && op.bias_off >= 0 && op.scale2_off >= 0 && op.shift2_off >= 0, "no weights or no bias");
      need(op.cin % 4 == 0 && op.cout % 4 == 0 && op.coutp % 32 == 0 && op.n_slabs > 0 && (int64_t)op.n_slabs * 32 >= op.cin && op.stride <= 2,
           "channel counts, K slabs or stride");
      need(op.prec == 0 || op.prec == 3, "arithmetic mode");
      need(!bad_w(op.w_off, image), "w_off past the weight region");
      need(!bad_w(op.bias_off, row), "bias_off past the weight region");
      need(!bad_w(op.scale2_off, (size_t)op.cin * 36), "scale2_off past the weight region");
      need(!bad_w(op.shift2_off, (size_t)op.cin * 4), "shift2_off past the weight region");
      need(wus_ok, "wus_off is not the [coutp] floats behind the bias");
    } else if (op.type == TA_OP_DWCONV) {
      need(op.w_off >= 0 && op.bias_off >= 0 && op.cin % 4 == 0 && op.kh == 3 && op.kw == 3, "no weights, no bias, or not 3x3");
      need(!bad_w(op.w_off, (size_t)op.cin * 36), "w_off past the weight region");
      need(!bad_w(op.bias_off, (size_t)op.cin * 4), "bias_off past the weight region");
    } else if (op.type != TA_OP_MAXPOOL && op.type != TA_OP_COPYCH) {
      return no("model blob: unknown op type %d (op %d)", op.type, oi);
    }
    if (why) return no("model blob: malformed op %d: %s", oi, why);

    const ta_tensor_desc &ti = td[op.in], &to = td[op.out];
    if (!view_ready(op.in)) return no("model blob: alias tensor %d used before its source %d (op %d)", op.in, ti.alias_of, oi);
    if (!set[op.in]) return no("model blob: op %d reads unset tensor %d", oi, op.in);
    if (op.type != TA_OP_CONV && (ti.fmt == TA_FMT_F16 || to.fmt == TA_FMT_F16))
      return no("model blob: op %d: only convs read and write half-float tensors", oi);
    if ((op.type == TA_OP_CONV || op.type == TA_OP_DWCONV) && ti.halo < op.pad)
      return no("model blob: op %d needs halo %d, tensor has %d", oi, op.pad, ti.halo);
    if (op.type == TA_OP_CONV) {
      const ta_k_geometry kg = ta_conv_k_geometry(op, ti.fmt);
      // grouped: runs on the split-role kernel only (uniform K walk, 128-channel tiles inside one group)
      if (op.groups > 1 && !(kg.uniform && op.n_slabs >= 2 && op.cout % op.groups == 0 && (op.cout / op.groups) % 128 == 0 && op.cout == op.coutp &&
                             op.in_ch_off % 32 == 0 && op.in_ch_off + (int64_t)op.groups * op.cin <= ti.channels && ti.fmt == ta_split_fmt_of(op.prec)))
        return no("model blob: op %d: unsupported grouped convolution", oi);
      if (op.pool && (op.out2 >= 0 || op.res >= 0 || op.groups > 1 || op.cin % 32 || op.coutp % 64))
        return no("model blob: op %d: unsupported conv + max-pool fusion", oi);
      if (ti.fmt == TA_FMT_F16 && (!kg.uniform || op.in_ch_off || op.groups > 1 || op.prec != 4))
        return no("model blob: op %d: a half-float tensor feeds whole-tensor convs of the f16 mode only", oi);
      if (ti.fmt != TA_FMT_F16 && (int64_t)op.kh * op.kw * (op.cin / 4) > (int64_t)op.n_slabs * 8)      // the K-offset table has 8 entries per slab
        return no("model blob: op %d has too few K slabs", oi);
    } else if (op.type == TA_OP_DWCONV) {
      if (op.in_ch_off || op.out_ch_off) return no("model blob: op %d: depthwise conv on a channel slice is not supported", oi);
      if (ti.unscale_off >= 0 || to.unscale_off >= 0) return no("model blob: inconsistent activation scales (op %d)", oi);
    } else if (op.type == TA_OP_RFSTEM) {
      if (oi != 0 || op.in != h.input_tensor || ti.alias_of != -2)
        return no("model blob: the RetinaFace front op must be op 0 on a shape-only input tensor (op %d)", oi);
    } else if (op.type == TA_OP_DWPW) {
      if (ti.halo < 1) return no("model blob: op %d (dw+pw) needs an input halo", oi);
      if (ti.fmt != TA_FMT_F32 || op.in_ch_off || op.cin > ti.channels) return no("model blob: op %d: unsupported dw+pw block", oi);
    }
    set[op.out] = 1;
    if (op.out2 >= 0) set[op.out2] = 1;

    const int lane = ta_op_lane(op);
    bool shared = lane == 3 || (lane && (op.type != TA_OP_CONV || ta_op_packed_ksplit(op) > 1 || op.pool));   // plain convs only
    for (int t : {op.in, op.res}) {
      if (t < 0) continue;
      if (writer_lane[t] && writer_lane[t] != lane) shared = true;          // a branch's result read outside the branch
      reader_lanes[t] |= 1 << lane;
    }
    for (int t : {op.out, op.out2}) {
      if (t < 0) continue;
      if (reader_lanes[t] & ~(1 << lane)) shared = true;                    // written while another lane may still read it
      if (writer_lane[t] && writer_lane[t] != lane) shared = true;
      if (lane) writer_lane[t] = lane;
      else if (reader_lanes[t] >> 1) shared = true;
    }
    if (shared) return no("model blob: an op lane (side stream) shares tensors with ops outside it (op %d)", oi);
  }
  for (int t = 0; t < T; ++t)
    if (!view_ready(t)) return no("model blob: alias tensor %d used before its source %d", t, td[t].alias_of);
  return TA_OK;
}

extern "C" {

int ta_program_check(int kind, const void* blob, size_t bytes, char* msg, size_t msg_capacity) {
  ta_program p;
  return ta_program_parse(kind, blob, bytes, &p, msg, msg_capacity);
}

int ta_model_load(ta_ctx* ctx, int kind, const void* blob, size_t bytes, ta_model** out) {
  ta_enter(ctx);
  if (!ctx || !blob || !out) return TA_E_INVALID;
  *out = nullptr;
  std::unique_ptr<ta_model> m(new ta_model());      // frees the weights too, on every return below
  char why[256];
  if (ta_program_parse(kind, blob, bytes, m.get(), why, sizeof(why)) != TA_OK) return ta_fail(ctx, TA_E_INVALID, "%s", why);
  const ta_blob_header& h = m->hdr;
  const char* weights = (const char*)blob + h.weights_off;
  m->ctx = ctx;
  m->kind = kind;
  m->unscale_host.resize(h.n_tensors);
  for (int t = 0; t < h.n_tensors; ++t)
    if (m->tdesc[t].unscale_off >= 0) {
      const float* v = (const float*)(weights + m->tdesc[t].unscale_off);
      m->unscale_host[t].assign(v, v + m->tdesc[t].channels);
    }
  m->tensor_read.assign(h.n_tensors, 0);
  for (auto& op : m->ops) {
    m->tensor_read[op.in] = 1;
    if (op.res >= 0) m->tensor_read[op.res] = 1;
    if ((op.type == TA_OP_CONV || op.type == TA_OP_DWPW) && (op.prec == 3 || op.prec == 4 || op.prec == 5)) m->has_half_ops = true;
  }
  for (int t = 0; t < h.n_tensors; ++t) {            // a view is read when its source is, and the other way round
    const int src = m->tdesc[t].alias_of;
    if (src >= 0 && (m->tensor_read[t] || m->tensor_read[src])) m->tensor_read[t] = m->tensor_read[src] = 1;
  }
  if (m->ops[0].type == TA_OP_RFSTEM) m->weights_host_small.assign(weights + m->ops[0].w_off, weights + m->ops[0].w_off + 448 * 4);
  hipError_t e = hipMalloc((void**)&m->weights_dev, h.weights_bytes ? h.weights_bytes : 16);
  if (e != hipSuccess) {
    m->weights_dev = nullptr;
    return ta_fail(ctx, TA_E_DEVICE, "hipMalloc(weights %lld) failed: %s", (long long)h.weights_bytes, hipGetErrorString(e));
  }
  e = hipMemcpy(m->weights_dev, weights, h.weights_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "weights upload failed: %s", hipGetErrorString(e));
  *out = m.release();
  return TA_OK;
}

void ta_model_free(ta_model* m) {
  ta_enter(m ? m->ctx : nullptr);
  if (!m) return;
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->ctx->amax_owner == m) m->ctx->amax_owner = nullptr;
  delete m;
}

int ta_model_kind(const ta_model* m) { return m ? m->kind : TA_E_INVALID; }

int ta_model_tensor_unscale(const ta_model* m, int tensor, float* out, int capacity) {
  if (!m || !out || tensor < 0 || tensor >= (int)m->tdesc.size()) return TA_E_INVALID;
  const int c = m->tdesc[tensor].channels;
  if (capacity < c) return TA_E_CAPACITY;
  for (int i = 0; i < c; ++i) out[i] = m->unscale_host[tensor].empty() ? 1.0f : m->unscale_host[tensor][i];
  return TA_OK;
}

}  // extern "C"
