// rt_chunked.h — how a host form pushes n units of work through one set of device buffers in chunks, so that the device memory of a call
// does not grow with n: the clocks of a call that may report rt_stats, the device buffers of one call, and the chunk driver.  It needs
// HIP's API, rt_stats and the error codes of include/rt_hip.h and a declared rt_api::fail, and nothing else of the project: every HIP
// call the driver makes is in this header, so a plain host compiler can build it against recording fakes (tests/host/chunked_check.cpp).
//   A unit is an element of a list, or one row of w pixels of a view (rows_per_chunk: whole rows of at most `chunk` pixels).
//   A row is one array of the call: IN rows are copied up in front of a chunk's step, OUT rows copied back behind it, SCRATCH rows are
//   device memory only.  Per chunk: the IN copies, step(first_unit, units, d_rows, st), the OUT copies, one hipStreamSynchronize.
#ifndef RT_CHUNKED_H
#define RT_CHUNKED_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include <chrono>

#include "../../include/rt_hip.h"

namespace rt_api {

int fail(int code, const char *fmt, ...);
#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

// GPU time between start() and stop() on a stream; the events are released on every way out
struct event_timer {
  hipEvent_t a = nullptr, b = nullptr;
  event_timer() = default;
  event_timer(const event_timer &) = delete;
  ~event_timer() { release(); }
  void release() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); a = b = nullptr; }
  hipError_t start(hipStream_t stream) {
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = hipEventRecord(a, stream);
    return e;
  }
  hipError_t stop(hipStream_t stream) { return hipEventRecord(b, stream); }
  hipError_t elapsed(float *ms) const { return hipEventElapsedTime(ms, a, b); }
};

// The clock of a call that may report rt_stats: host time from its construction, GPU time on `stream` between start() and finish().
// Without `stats` (most calls) it creates no event and waits for nothing.
struct stats_clock {
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  event_timer timer;
  hipStream_t stream = nullptr;
  double host_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); }
  int start(const rt_stats *stats, hipStream_t on) {
    stream = on;
    if (stats) HIP_TRY(timer.start(stream));
    return RT_OK;
  }
  // waits for the stream; *stats = {kernel_ms, pixels, total_ms}, every other field zero
  int finish(rt_stats *stats, uint64_t pixels) {
    if (!stats) return RT_OK;
    HIP_TRY(timer.stop(stream));
    HIP_TRY(hipEventSynchronize(timer.b));
    float ms = 0.f;
    HIP_TRY(timer.elapsed(&ms));
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = ms;
    stats->pixels = pixels;
    stats->total_ms = host_ms();
    return RT_OK;
  }
};

// device buffers of one call, released on every way out
template <int N> struct device_bufs {
  void *p[N] = {};
  device_bufs() = default;
  device_bufs(const device_bufs &) = delete;
  ~device_bufs() { for (void *q : p) if (q) (void)hipFree(q); }
};

// One array of a chunked call.  IN, OUT: `host` is the whole array, `each` its bytes per unit; without a host pointer the row gets no
// buffer and the step sees NULL for it.  SCRATCH: each * units-per-chunk + flat bytes of device memory (flat: a size that is no multiple
// of the units, like the workspace of an ordering); none where that is 0.
enum row_dir { ROW_IN, ROW_OUT, ROW_SCRATCH };
struct chunk_row { const void *host; size_t each; row_dir dir; size_t flat; };
inline chunk_row row_in(const void *host, size_t each) { return chunk_row{host, each, ROW_IN, 0}; }
inline chunk_row row_out(void *host, size_t each) { return chunk_row{host, each, ROW_OUT, 0}; }
inline chunk_row row_scratch(size_t each, size_t flat = 0) { return chunk_row{nullptr, each, ROW_SCRATCH, flat}; }
constexpr int RT_CHUNK_ROWS = 8;

// units per chunk of a call over n: the driver's own figure, for a caller that sizes a SCRATCH row's flat part by it
inline uint64_t units_per_chunk(uint64_t n, uint64_t chunk) { return n < chunk ? n : chunk; }
// a view of w x h pixels in chunks of whole rows of at most `chunk` pixels; a longer row is its own chunk
inline uint32_t rows_per_chunk(uint64_t chunk, uint32_t w, uint32_t h) {
  const uint64_t rows = chunk / w;
  return rows < 1u ? 1u : rows > h ? h : (uint32_t)rows;
}

// n units in chunks of at most `chunk` on `stream`, which the caller has made ready.  step(first_unit, units, d_rows, st) -> an error
// code: the chunk's launches, on device buffers that hold units [first_unit, first_unit + units) from their start; st is NULL when the
// call reports no stats (kernel_ms NULL), else the step leaves its GPU time in st->kernel_ms, and *kernel_ms is the sum over the chunks.
// Synchronous; every buffer is released on every way out.
template <typename Step>
int chunked_call(hipStream_t stream, uint64_t n, uint64_t chunk, const chunk_row *rows, int n_rows, double *kernel_ms, Step step) {
  if (n_rows > RT_CHUNK_ROWS) return fail(RT_ERR_INVALID, "a chunked call has at most %d arrays", RT_CHUNK_ROWS);
  chunk = units_per_chunk(n, chunk);
  device_bufs<RT_CHUNK_ROWS> mem;
  for (int i = 0; i < n_rows; i++) {
    const size_t bytes = rows[i].dir == ROW_SCRATCH ? (size_t)chunk * rows[i].each + rows[i].flat : rows[i].host ? (size_t)chunk * rows[i].each : 0;
    if (bytes) HIP_TRY(hipMalloc(&mem.p[i], bytes));
  }
  if (kernel_ms) *kernel_ms = 0.0;
  for (uint64_t first = 0; chunk != 0 && first < n; first += chunk) {
    const uint64_t m = n - first < chunk ? n - first : chunk;
    for (int i = 0; i < n_rows; i++)
      if (mem.p[i] && rows[i].dir == ROW_IN)
        HIP_TRY(hipMemcpyAsync(mem.p[i], (const uint8_t *)rows[i].host + first * rows[i].each, (size_t)m * rows[i].each, hipMemcpyHostToDevice, stream));
    rt_stats st;
    st.kernel_ms = 0.0;
    if (int rc = step(first, m, (void *const *)mem.p, kernel_ms ? &st : nullptr)) return rc;
    if (kernel_ms) *kernel_ms += st.kernel_ms;
    for (int i = 0; i < n_rows; i++)
      if (mem.p[i] && rows[i].dir == ROW_OUT)
        HIP_TRY(hipMemcpyAsync((uint8_t *)rows[i].host + first * rows[i].each, mem.p[i], (size_t)m * rows[i].each, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return RT_OK;
}

}  // namespace rt_api

#endif
