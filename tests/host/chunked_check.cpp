// chunked_check.cpp — the chunk driver of the host forms (csrc/rt_chunked.h: chunked_call, rows_per_chunk), checked on a CPU.  The HIP
// functions the header calls are defined HERE, as recorders: each appends one entry to a log, hipMalloc hands out handles in call order;
// no HIP runtime is linked.  Every scenario drives the driver the way a host form does and compares the calls with the expected ones
// written below:
//   malloc(aK,B)      allocation K of B bytes            free(aK)
//   up(aK<-hJ+O,B)    B bytes of host array J from offset O into allocation K         down(hJ+O<-aK,B)   the way back
//   step(F,U)         the chunk's step sees first_unit F and U units                  sync               the stream is drained
// Then a failure is injected at the third hipMalloc, at the second chunk's copy-in, in a step and at the final synchronise: the driver
// returns the error, starts nothing after it and has freed everything.  Exit status 1 with the differing scenarios on stderr.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I<csrc> chunked_check.cpp
#include "rt_chunked.h"

#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

using namespace rt_api;

namespace {
std::string g_log;                                        // every call, in order
std::vector<int> g_freed;                                 // per allocation: how often it was freed
int g_failures = 0, g_bad_frees = 0;
int g_mallocs = 0, g_ups = 0, g_syncs = 0;                // calls so far, of the kinds a failure can be injected into
int g_fail_malloc = 0, g_fail_up = 0, g_fail_sync = 0;    // the call of its kind (1-based) that fails; 0: none
char g_host[3][1024];                                     // the host arrays h0, h1, h2
hipStream_t const STREAM = (hipStream_t)(uintptr_t)0x57;

void *handle(int k) { return (void *)(uintptr_t)(0x100000u * (unsigned)(k + 1)); }
std::string alloc_name(const void *p) {
  const uintptr_t a = (uintptr_t)p;
  return (a % 0x100000u == 0 && a / 0x100000u >= 1 && a / 0x100000u <= g_freed.size()) ? "a" + std::to_string(a / 0x100000u - 1) : "a?";
}
std::string host_name(const void *p) {
  for (int j = 0; j < 3; j++)
    if ((const char *)p >= g_host[j] && (const char *)p < g_host[j] + sizeof g_host[j]) return "h" + std::to_string(j) + "+" + std::to_string((const char *)p - g_host[j]);
  return "h?";
}
void say(const std::string &t) { g_log += (g_log.empty() ? "" : " ") + t; }
void check(bool ok, const char *scenario, const char *what) { if (!ok) { fprintf(stderr, "%s: %s\n", scenario, what); g_failures++; } }

void reset() {
  g_log.clear(); g_freed.clear();
  g_mallocs = g_ups = g_syncs = g_bad_frees = 0;
  g_fail_malloc = g_fail_up = g_fail_sync = 0;
}
// the log is the expected one, and every allocation was freed exactly once
void expect(const char *scenario, const std::string &want) {
  if (g_log != want) { fprintf(stderr, "%s:\n  expected  %s\n  got       %s\n", scenario, want.c_str(), g_log.c_str()); g_failures++; }
  for (size_t k = 0; k < g_freed.size(); k++) check(g_freed[k] == 1, scenario, "an allocation was not freed exactly once");
  check(g_bad_frees == 0, scenario, "a pointer that was never allocated was freed");
}
}  // namespace

// ---- the recorders
int rt_api::fail(int code, const char *, ...) { return code; }
extern "C" {
const char *hipGetErrorString(hipError_t) { return "injected"; }
hipError_t hipMalloc(void **p, size_t bytes) {
  if (++g_mallocs == g_fail_malloc) { say("malloc!"); *p = nullptr; return hipErrorOutOfMemory; }
  *p = handle((int)g_freed.size());
  g_freed.push_back(0);
  say("malloc(" + alloc_name(*p) + "," + std::to_string(bytes) + ")");
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  const std::string n = alloc_name(p);
  if (n == "a?") { g_bad_frees++; return hipErrorInvalidValue; }
  g_freed[(size_t)std::stoi(n.substr(1))]++;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  if (stream != STREAM) say("stream?");
  if (kind == hipMemcpyHostToDevice) {
    if (++g_ups == g_fail_up) { say("up!"); return hipErrorInvalidValue; }
    say("up(" + alloc_name(dst) + "<-" + host_name(src) + "," + std::to_string(bytes) + ")");
  } else if (kind == hipMemcpyDeviceToHost) {
    say("down(" + host_name(dst) + "<-" + alloc_name(src) + "," + std::to_string(bytes) + ")");
  } else {
    say("copy?");
  }
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
  if (stream != STREAM) say("stream?");
  if (++g_syncs == g_fail_sync) { say("sync!"); return hipErrorLaunchFailure; }
  say("sync");
  return hipSuccess;
}
// the clocks of the header: no scenario uses one
hipError_t hipEventCreate(hipEvent_t *) { say("event?"); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { say("event?"); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { say("event?"); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { say("event?"); return hipSuccess; }
hipError_t hipEventElapsedTime(float *, hipEvent_t, hipEvent_t) { say("event?"); return hipSuccess; }
}

namespace {
// A list as a host form hands it over: h0 goes up (4 bytes per unit), h1 comes back (2), an IN row and an OUT row without a host
// pointer, scratch of 3 bytes per unit and 5 more, and scratch of nothing.  The step sees the allocations in row order and NULL for
// the rows that have none; it reports 1.5 ms where it is asked to.  fail_step: the step (1-based) that returns -7.
int run_list(const char *scenario, uint64_t n, bool timed, double *kernel_ms, int fail_step = 0) {
  const chunk_row rows[6] = {row_in(g_host[0], 4u), row_out(g_host[1], 2u), row_in(nullptr, 8u), row_scratch(3u, 5u), row_out(nullptr, 8u), row_scratch(0u)};
  int steps = 0;
  return chunked_call(STREAM, n, 4u, rows, 6, timed ? kernel_ms : nullptr, [&](uint64_t first, uint64_t units, void *const *d, rt_stats *st) {
    say("step(" + std::to_string(first) + "," + std::to_string(units) + ")");
    check(d[0] == handle(0) && d[1] == handle(1) && d[3] == handle(2), scenario, "the step does not see the allocations in row order");
    check(!d[2] && !d[4] && !d[5], scenario, "a row without a host pointer, or scratch of no bytes, is not NULL in the step");
    check((st != nullptr) == timed, scenario, "st is not NULL exactly when the call reports no stats");
    if (st) st->kernel_ms = 1.5;
    return ++steps == fail_step ? -7 : 0;
  });
}

const std::string A4 = "malloc(a0,16) malloc(a1,8) malloc(a2,17)";      // the allocations of a chunk of 4 units
const std::string C0 = " up(a0<-h0+0,16) step(0,4) down(h1+0<-a1,8) sync";

void lists() {
  double ms = -1.0;
  reset();
  check(run_list("n = 1", 1, false, nullptr) == RT_OK, "n = 1", "an error");
  expect("n = 1", "malloc(a0,4) malloc(a1,2) malloc(a2,8) up(a0<-h0+0,4) step(0,1) down(h1+0<-a1,2) sync");
  reset();
  check(run_list("n = 4", 4, true, &ms) == RT_OK && ms == 1.5, "n = 4", "an error, or kernel_ms is not the chunk's");
  expect("n = 4", A4 + C0);
  reset();
  check(run_list("n = 5", 5, false, nullptr) == RT_OK, "n = 5", "an error");
  expect("n = 5", A4 + C0 + " up(a0<-h0+16,4) step(4,1) down(h1+8<-a1,2) sync");
  reset();
  check(run_list("n = 9", 9, true, &ms) == RT_OK && ms == 4.5, "n = 9", "an error, or kernel_ms is not the sum over the chunks");
  expect("n = 9", A4 + C0 + " up(a0<-h0+16,16) step(4,4) down(h1+8<-a1,8) sync up(a0<-h0+32,4) step(8,1) down(h1+16<-a1,2) sync");
}

// A view of w = 3 by h = 5 pixels as a host form hands it over: a unit is one row of 3 pixels, the band workspace is scratch of 48
// bytes per pixel, rgb (24 per pixel) and rgba (4) come back
void views() {
  const uint32_t w = 3, h = 5;
  check(rows_per_chunk(3, w, h) == 1 && rows_per_chunk(5, w, h) == 1 && rows_per_chunk(6, w, h) == 2 && rows_per_chunk(8, w, h) == 2, "rows_per_chunk", "whole rows of at most `chunk` pixels");
  check(rows_per_chunk(2, w, h) == 1, "rows_per_chunk", "a row longer than a chunk is its own chunk");
  check(rows_per_chunk(1u << 18, w, h) == 5 && rows_per_chunk(15, w, h) == 5, "rows_per_chunk", "at most the view's rows");
  const chunk_row rows[3] = {row_scratch(w * 48u), row_out(g_host[0], w * 24u), row_out(g_host[1], w * 4u)};
  auto step = [&](uint64_t y, uint64_t m, void *const *d, rt_stats *) {
    say("step(" + std::to_string(y) + "," + std::to_string(m) + ")");
    check(d[0] == handle(0) && d[1] == handle(1) && d[2] == handle(2), "view", "the step does not see the allocations in row order");
    return 0;
  };
  reset();
  check(chunked_call(STREAM, h, rows_per_chunk(3, w, h), rows, 3, nullptr, step) == RT_OK, "view, 1 row per chunk", "an error");
  std::string want = "malloc(a0,144) malloc(a1,72) malloc(a2,12)";
  for (uint32_t y = 0; y < h; y++)
    want += " step(" + std::to_string(y) + ",1) down(h0+" + std::to_string(72 * y) + "<-a1,72) down(h1+" + std::to_string(12 * y) + "<-a2,12) sync";
  expect("view, 1 row per chunk", want);
  reset();
  check(chunked_call(STREAM, h, rows_per_chunk(7, w, h), rows, 3, nullptr, step) == RT_OK, "view, 2 rows per chunk", "an error");
  expect("view, 2 rows per chunk", "malloc(a0,288) malloc(a1,144) malloc(a2,24)"
                                   " step(0,2) down(h0+0<-a1,144) down(h1+0<-a2,24) sync"
                                   " step(2,2) down(h0+144<-a1,144) down(h1+24<-a2,24) sync"
                                   " step(4,1) down(h0+288<-a1,72) down(h1+48<-a2,12) sync");
}

// the driver returns the error, starts nothing after it (the log ends at the failing call) and has freed everything (expect)
void failures() {
  reset(); g_fail_malloc = 3;
  check(run_list("the third hipMalloc fails", 9, false, nullptr) == RT_ERR_DEVICE, "the third hipMalloc fails", "not RT_ERR_DEVICE");
  expect("the third hipMalloc fails", "malloc(a0,16) malloc(a1,8) malloc!");
  reset(); g_fail_up = 2;
  check(run_list("the second chunk's copy-in fails", 9, false, nullptr) == RT_ERR_DEVICE, "the second chunk's copy-in fails", "not RT_ERR_DEVICE");
  expect("the second chunk's copy-in fails", A4 + C0 + " up!");
  reset();
  check(run_list("the second step fails", 9, false, nullptr, 2) == -7, "the second step fails", "not the step's own code");
  expect("the second step fails", A4 + C0 + " up(a0<-h0+16,16) step(4,4)");
  reset(); g_fail_sync = 2;
  check(run_list("the final synchronise fails", 5, false, nullptr) == RT_ERR_DEVICE, "the final synchronise fails", "not RT_ERR_DEVICE");
  expect("the final synchronise fails", A4 + C0 + " up(a0<-h0+16,4) step(4,1) down(h1+8<-a1,2) sync!");
  // more rows than the driver holds: refused before anything is allocated
  reset();
  chunk_row many[RT_CHUNK_ROWS + 1];
  for (chunk_row &r : many) r = row_scratch(1u);
  check(chunked_call(STREAM, 4, 4, many, RT_CHUNK_ROWS + 1, nullptr, [](uint64_t, uint64_t, void *const *, rt_stats *) { return 0; }) == RT_ERR_INVALID, "too many rows", "not RT_ERR_INVALID");
  expect("too many rows", "");
}
}  // namespace

int main() {
  lists();
  views();
  failures();
  if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures); return 1; }
  printf("chunked_check: the chunk driver makes the expected HIP calls\n");
  return 0;
}
