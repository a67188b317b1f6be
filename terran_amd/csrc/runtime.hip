// Context, error text, scratch and pinned staging, the f16x3 range flag, HIP-event profiling and timers.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "ta_internal.h"

int ta_fail(ta_ctx* ctx, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

int ta_scratch(ta_ctx* ctx, size_t bytes, void** out) {
  if (bytes > ctx->scratch_bytes) {
    // the old block may still be read by queued kernels: drain first
    TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    size_t want = bytes + bytes / 4 + (1 << 20);
    TA_HIP(ctx, hipMalloc(&ctx->scratch, want));
    ctx->scratch_bytes = want;
  }
  *out = ctx->scratch;
  return TA_OK;
}

int ta_pinned(ta_ctx* ctx, size_t bytes, void** out) {
  if (bytes > ctx->pinned_bytes) {
    TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
    size_t want = bytes + bytes / 4 + (1 << 16);
    TA_HIP(ctx, hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault));
    ctx->pinned_bytes = want;
  }
  *out = ctx->pinned;
  return TA_OK;
}

// ---- f16x3 range flag -----------------------------------------------------------------------------
int ta_range_enqueue(ta_ctx* ctx) {
  TA_HIP(ctx, hipMemcpyAsync(ctx->range_flag_host, ctx->range_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  return TA_OK;
}

int ta_range_check(ta_ctx* ctx) {
  if (!*ctx->range_flag_host) return TA_OK;
  *ctx->range_flag_host = 0;
  TA_HIP(ctx, hipMemsetAsync(ctx->range_flag, 0, sizeof(int), ctx->stream));
  return ta_fail(ctx, TA_E_RANGE, "f16x3: an activation exceeded the half-float range (|x| > 65504); run this input in the f32 or bf16x3 mode");
}

// End of a task entry point whose post-processing returned `rc`: garbage maps of an overflowed network can make the grouping /
// selection fail in their own ways (TA_E_OVERFLOW with > 65535 "peaks", ...); the caller must then hear TA_E_RANGE -- the error it
// can act on (re-run on the exact-f32 twin) -- and the flag must not survive into the next, unrelated call.
int ta_range_finish(ta_ctx* ctx, int rc) {
  if (rc != TA_OK && rc != TA_E_CAPACITY) (void)hipStreamSynchronize(ctx->stream);    // error paths may have returned before their sync
  const int rr = ta_range_check(ctx);
  return rr != TA_OK ? rr : rc;
}

// ---- profiling ---------------------------------------------------------------------------------
static hipEvent_t get_event(ta_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

ta_prof_scope::ta_prof_scope(ta_ctx* c, int k, double w) : ctx(c), klass(k), work(w) {
  ctx->cur_kernel = nullptr;          // whatever launch noted its instance last belongs to an EARLIER scope (also while profiling was off)
  if (!ctx->profiling) return;
  a = get_event(ctx);
  b = get_event(ctx);
  if (a) (void)hipEventRecord(a, ctx->stream);
}

ta_prof_scope::~ta_prof_scope() {
  if (!ctx->profiling || !a || !b) {
    ctx->cur_kernel = nullptr;
    return;
  }
  (void)hipEventRecord(b, ctx->stream);
  ctx->pending.push_back({a, b, klass, ctx->cur_kernel});
  ctx->cur_kernel = nullptr;
  ctx->prof[klass].launches += 1;
  ctx->prof[klass].work += work;
}

void ta_drain_profile(ta_ctx* ctx) {
  if (ctx->pending.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& pe : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
      ctx->prof[pe.klass].ms += ms;
      if (pe.kernel) ctx->kernel_ms[*pe.kernel] += ms;
    }
    ctx->event_pool.push_back(pe.a);
    ctx->event_pool.push_back(pe.b);
  }
  ctx->pending.clear();
}

extern "C" {

const char* ta_version(void) { return "terran_amd 0.1.0 (gfx950)"; }

int ta_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ta_device_pci_bus_id(int device_id, char* out, int capacity) {
  if (!out || capacity < 16) return TA_E_INVALID;
  out[0] = 0;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return TA_E_DEVICE;
  if (hipDeviceGetPCIBusId(out, capacity, device_id) != hipSuccess) return TA_E_DEVICE;
  return TA_OK;
}

int ta_ctx_create(int device_id, ta_ctx** out) {
  if (!out) return TA_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return TA_E_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return TA_E_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return TA_E_DEVICE;   // this library is gfx950-only
  if (hipSetDevice(device_id) != hipSuccess) return TA_E_DEVICE;
  // Host threads BLOCK in their stream syncs instead of spinning: every task thread (detect / embed / pose per lane, 12+ per
  // GPU) ends each call in hipStreamSynchronize, and the runtime's default wait polls the completion signal from user space for
  // as long as the stream runs -- ~6 cores busy per rank doing nothing (0.085 CPU-seconds per 13.5 ms step, round 5).  With
  // this flag the runtime polls for ~100 us (short kernels still return at once) and then sleeps on the signal's interrupt.
  // TERRAN_AMD_SPIN_WAIT=1 keeps the spinning wait (latency probes).
  {
    const char* spin = getenv("TERRAN_AMD_SPIN_WAIT");
    if (!(spin && spin[0] && spin[0] != '0')) {
      (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
      (void)hipGetLastError();          // a runtime that refuses the flag on an already active device must not leave an error for the first launch check
    }
  }
  ta_ctx* ctx = new ta_ctx();
  ctx->device = device_id;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return TA_E_DEVICE;
  }
  (void)hipEventCreate(&ctx->t0);
  (void)hipEventCreate(&ctx->t1);
  const size_t flag_bytes = sizeof(int) * (TA_AMAX_SLOT0 + 2 * TA_AMAX_OPS);
  if (hipMalloc((void**)&ctx->range_flag, flag_bytes) != hipSuccess || hipMemset(ctx->range_flag, 0, flag_bytes) != hipSuccess ||
      hipHostMalloc((void**)&ctx->range_flag_host, sizeof(int), hipHostMallocDefault) != hipSuccess) {
    if (ctx->range_flag) (void)hipFree(ctx->range_flag);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return TA_E_DEVICE;
  }
  *ctx->range_flag_host = 0;
  // measurement aid for tools/ (the shipped path leaves it unset)
  if (const char* e = getenv("TA_CONV_PREFER")) ctx->conv_force = atoi(e);
#ifdef TA_CONV_TRACE
  if (const char* e = getenv("TA_CONV_TRACE_BLOCK")) ctx->conv_trace_block = atoi(e);
#endif
  *out = ctx;
  return TA_OK;
}

void ta_ctx_destroy(ta_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ta_drain_profile(ctx);
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  if (ctx->t0) (void)hipEventDestroy(ctx->t0);
  if (ctx->t1) (void)hipEventDestroy(ctx->t1);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pose_wphase) (void)hipFree(ctx->pose_wphase);
  if (ctx->jpeg_enc_dev) (void)hipFree(ctx->jpeg_enc_dev);
  if (ctx->jpeg_enc_out) (void)hipHostFree(ctx->jpeg_enc_out);
  if (ctx->yuv_in) (void)hipFree(ctx->yuv_in);
  ta_pose_free_big(ctx);
  if (ctx->range_flag) (void)hipFree(ctx->range_flag);
  if (ctx->range_flag_host) (void)hipHostFree(ctx->range_flag_host);
  for (auto& e : ctx->frame_cache) (void)hipFree(e.second);
  for (int i = 0; i < 2; ++i) {
    if (ctx->side_stream[i]) {
      (void)hipStreamSynchronize(ctx->side_stream[i]);
      (void)hipStreamDestroy(ctx->side_stream[i]);
    }
    if (ctx->side_fork[i]) (void)hipEventDestroy(ctx->side_fork[i]);
    if (ctx->side_join[i]) (void)hipEventDestroy(ctx->side_join[i]);
  }
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* ta_last_error(const ta_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ta_debug_range_check(ta_ctx* ctx) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  TA_TRY(ta_range_enqueue(ctx));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ta_range_check(ctx);
}

int ta_ctx_sync(ta_ctx* ctx) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TA_OK;
}

int ta_profile_enable(ta_ctx* ctx, int on) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (!on) ta_drain_profile(ctx);
  ctx->profiling = on != 0;
  return TA_OK;
}

int ta_profile_reset(ta_ctx* ctx) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  ta_drain_profile(ctx);
  for (auto& p : ctx->prof) p = ta_prof_class();
  return TA_OK;
}

int ta_profile_read(ta_ctx* ctx, int klass, double* ms, int64_t* launches, double* work) {
  ta_enter(ctx);
  if (!ctx || klass < 0 || klass > 3) return TA_E_INVALID;
  ta_drain_profile(ctx);
  if (ms) *ms = ctx->prof[klass].ms;
  if (launches) *launches = ctx->prof[klass].launches;
  if (work) *work = ctx->prof[klass].work;
  return TA_OK;
}

int ta_timer_start(ta_ctx* ctx) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  TA_HIP(ctx, hipEventRecord(ctx->t0, ctx->stream));
  return TA_OK;
}

int ta_timer_stop(ta_ctx* ctx, double* ms) {
  ta_enter(ctx);
  if (!ctx || !ms) return TA_E_INVALID;
  TA_HIP(ctx, hipEventRecord(ctx->t1, ctx->stream));
  TA_HIP(ctx, hipEventSynchronize(ctx->t1));
  float f = 0.f;
  TA_HIP(ctx, hipEventElapsedTime(&f, ctx->t0, ctx->t1));
  *ms = f;
  return TA_OK;
}

}  // extern "C"
