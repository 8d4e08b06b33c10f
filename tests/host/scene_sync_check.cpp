// scene_sync_check.cpp — the stream-ordering rules of a resident scene (csrc/rt_scene_sync.h: R1-R6), checked on a CPU.  The HIP
// functions the header calls are defined HERE, as recorders: each appends one line to a log and hands out handles in creation order; no
// HIP runtime is linked.  Every scenario drives a scene_sync the way rt_scene.hip does and compares the calls of each step with the
// expected ones written below: rec(E,X) records event E on stream X, wait(X,E) makes stream X wait for E, sync(E) is a host wait for E,
// drain a device synchronise.  A, B: caller streams; S: the scene's side stream.  Calls that only create or destroy are checked by the
// lifetime scenario, not per step.  Exit status 1 with the differing steps on stderr.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I<csrc> scene_sync_check.cpp
#include "rt_scene_sync.h"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>

using namespace rt_api;

namespace {
struct call { const char *what; void *event; void *stream; };
std::vector<call> g_log;                                  // every call, in order
size_t g_seen = 0;                                        // ... up to here the steps so far have looked
uintptr_t g_handles = 0;
std::map<void *, int> g_events, g_streams;                // handle -> 0 alive, n destroyed n times
std::vector<std::pair<void *, int>> g_pinned;             // ... and per allocation (malloc may hand an address out again)
int g_failures = 0;

hipStream_t const A = (hipStream_t)(uintptr_t)0xA0, B = (hipStream_t)(uintptr_t)0xB0;

hipError_t logged(const char *what, void *event, void *stream) { g_log.push_back(call{what, event, stream}); return hipSuccess; }

std::string event_name(const scene_sync &y, void *e) {
  for (int b = 0; b < 2; b++) {
    if (e == y.old_done[b].h) return "OLD" + std::to_string(b);
    if (e == y.prep[b].ev.h) return "PREP" + std::to_string(b);
  }
  if (e == y.tex_before.h) return "TEXB";
  if (e == y.tex.ev.h) return "TEXD";
  for (uint32_t i = 0; i < pinned_ring::n_slots; i++) {
    if (e == y.moves.slots[i].read.h) return "SLOT" + std::to_string(i);
    if (e == y.texels.slots[i].read.h) return "TSLOT" + std::to_string(i);
  }
  return "event?";
}
std::string stream_name(const scene_sync &y, void *s) { return s == A ? "A" : s == B ? "B" : (s && s == y.side.h) ? "S" : "stream?"; }

// the ordering calls since the last step, in the notation of the expected logs ("-": none)
std::string calls_since(const scene_sync &y) {
  std::string out;
  for (; g_seen < g_log.size(); g_seen++) {
    const call &c = g_log[g_seen];
    const std::string w = c.what;
    std::string t;
    if (w == "rec") t = "rec(" + event_name(y, c.event) + "," + stream_name(y, c.stream) + ")";
    else if (w == "wait") t = "wait(" + stream_name(y, c.stream) + "," + event_name(y, c.event) + ")";
    else if (w == "sync") t = "sync(" + event_name(y, c.event) + ")";
    else if (w == "drain") t = "drain";
    else continue;
    out += (out.empty() ? "" : " ") + t;
  }
  return out.empty() ? "-" : out;
}

void expect(const scene_sync &y, const char *scenario, const char *step, const std::string &want) {
  const std::string got = calls_since(y);
  if (got == want) return;
  fprintf(stderr, "%s, %s:\n  expected  %s\n  got       %s\n", scenario, step, want.c_str(), got.c_str());
  g_failures++;
}
void check(bool ok, const char *what) { if (!ok) { fprintf(stderr, "%s\n", what); g_failures++; } }
void must(hipError_t e) { if (e != hipSuccess) { fprintf(stderr, "a call of the module failed\n"); exit(2); } }

// a scene as rt_scene.hip drives it
struct scene {
  scene_sync y;
  uint64_t gen = 1;
  scene() { must(y.moves.make(64u)); }
  void launch(hipStream_t x) { must(y.before_launch(x, gen)); y.note_launch(x); }
  void move() {
    must(y.ensure_side());
    const uint64_t G = ++gen;
    must(y.begin_generation(G));
    pinned_ring::slot *slot = nullptr;
    must(y.moves.acquire(&slot));
    must(y.moves.done(slot, y.side.h));
    must(y.end_generation(G));
  }
  void edit(hipStream_t x) { must(y.begin_edit(x)); must(y.end_edit(x)); }
};

void one_stream() {
  const char *n = "a. one stream";
  scene s;
  s.launch(A); expect(s.y, n, "launch A", "-");
  check(!s.y.side && !s.y.old_done[0] && !s.y.prep[1].ev && !s.y.tex_before && !s.y.tex.ev, "R6: an event or the side stream exists before the first move or edit");
  s.move();    expect(s.y, n, "move->2", "rec(OLD1,A) rec(SLOT0,S) rec(PREP0,S)");
  check(!s.y.tex_before && !s.y.tex.ev, "R6: a texel event exists before the first edit");
  s.launch(A); expect(s.y, n, "launch A (first of 2)", "wait(A,PREP0)");
  s.launch(A); expect(s.y, n, "launch A (second of 2)", "-");
  s.move();    expect(s.y, n, "move->3", "rec(OLD0,A) wait(S,OLD1) rec(SLOT1,S) rec(PREP1,S)");
  s.launch(A); expect(s.y, n, "launch A (3)", "wait(A,PREP1)");
  s.move();    expect(s.y, n, "move->4", "rec(OLD1,A) wait(S,OLD0) rec(SLOT2,S) rec(PREP0,S)");
  s.move();    expect(s.y, n, "move->5, nothing launched between", "wait(S,OLD1) rec(SLOT3,S) rec(PREP1,S)");
  s.launch(A); expect(s.y, n, "launch A (5)", "wait(A,PREP1)");
}

void two_streams() {
  const char *n = "b. two streams";
  scene s;
  s.launch(A); s.launch(B); expect(s.y, n, "launch A; launch B", "-");
  s.move();    expect(s.y, n, "move->2", "drain rec(SLOT0,S) rec(PREP0,S)");
  s.launch(A); expect(s.y, n, "launch A", "wait(A,PREP0)");
  s.launch(B); expect(s.y, n, "launch B", "wait(B,PREP0)");
  s.move();    expect(s.y, n, "move->3", "drain rec(SLOT1,S) rec(PREP1,S)");
}

void edits_across_streams() {
  const char *n = "c. edits across streams, no move";
  scene s;
  s.launch(A); expect(s.y, n, "launch A", "-");
  s.edit(B);   expect(s.y, n, "edit on B", "rec(TEXB,A) wait(B,TEXB) rec(TEXD,B)");
  check(!s.y.side && !s.y.old_done[0] && !s.y.prep[0].ev, "R6: a move's event or the side stream exists before the first move");
  s.launch(A); expect(s.y, n, "launch A (first behind the edit)", "wait(A,TEXD)");
  s.launch(A); expect(s.y, n, "launch A (second)", "-");
  s.launch(B); expect(s.y, n, "launch B", "-");
  s.edit(A);   expect(s.y, n, "edit on A", "drain wait(A,TEXD) rec(TEXD,A)");
  s.launch(B); expect(s.y, n, "launch B (behind the second edit)", "wait(B,TEXD)");
}

void edits_on_the_launches_stream() {
  const char *n = "d. edits on the launches' stream";
  scene s;
  s.edit(A);   expect(s.y, n, "edit on A before any launch", "rec(TEXD,A)");
  s.launch(A); expect(s.y, n, "launch A", "-");
  s.edit(A);   expect(s.y, n, "edit on A", "rec(TEXD,A)");
  s.launch(A); expect(s.y, n, "launch A (behind the second edit)", "-");
}

void ring() {
  const char *n = "e. ring";
  const size_t slot_bytes = 4096u;
  scene_sync y;
  must(y.moves.make(slot_bytes));
  uint8_t *h[pinned_ring::n_slots];
  for (uint32_t i = 0; i < pinned_ring::n_slots; i++) {
    pinned_ring::slot *g = nullptr;
    must(y.moves.acquire(&g));
    must(y.moves.done(g, A));
    h[i] = g->h;
    if (i) check(h[i] == h[i - 1] + slot_bytes, "e. ring: two slots in a row are not slot_bytes apart");
  }
  std::string want;
  for (uint32_t i = 0; i < pinned_ring::n_slots; i++) want += (i ? " rec(SLOT" : "rec(SLOT") + std::to_string(i) + ",A)";
  expect(y, n, "sixteen acquire / done pairs", want);
  pinned_ring::slot *g = nullptr;
  must(y.moves.acquire(&g));
  expect(y, n, "the seventeenth acquire", "sync(SLOT0)");
  check(g->h == h[0], "e. ring: the seventeenth slot is not the first");
}

// every handle made so far has been destroyed exactly once
void all_released(const char *n, size_t events, size_t streams, size_t pools) {
  for (const auto &e : g_events) check(e.second == 1, "f. lifetime: an event was not destroyed exactly once");
  for (const auto &s : g_streams) check(s.second == 1, "f. lifetime: a stream was not destroyed exactly once");
  for (const auto &p : g_pinned) check(p.second == 1, "f. lifetime: a pinned pool was not freed exactly once");
  if (g_events.size() != events || g_streams.size() != streams || g_pinned.size() != pools) {
    fprintf(stderr, "f. lifetime, %s: %zu events, %zu streams, %zu pools made; expected %zu, %zu, %zu\n", n, g_events.size(), g_streams.size(), g_pinned.size(), events, streams, pools);
    g_failures++;
  }
  g_events.clear(); g_streams.clear(); g_pinned.clear();
}

void lifetime() {
  all_released("scenarios a to e", 16u * 5u + 4u * 2u + 2u * 2u, 2u, 5u);    // (a, b: a ring and a move's events; c, d: a ring and an edit's; e: a ring)
  { scene s; s.launch(A); }
  all_released("a scene that never moved and never edited", 16u, 0u, 1u);
  {
    scene s;
    must(s.y.texels.make(256u));
    s.launch(A); s.move(); s.edit(B); s.launch(B); s.move();
    event moved(std::move(s.y.tex_before));                  // (a moved-from event owns nothing)
    check(!s.y.tex_before && moved, "f. lifetime: a move did not hand the event over");
  }
  all_released("a scene that moved and edited", 32u + 4u + 2u, 1u, 2u);
}
}  // namespace

// ------------------------------------------------------------------------------------ the recorders
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags) {
  check(flags == hipEventDisableTiming, "an event was made with timing");
  *event = (hipEvent_t)(++g_handles);
  g_events[*event] = 0;
  return logged("event+", *event, nullptr);
}
hipError_t hipEventDestroy(hipEvent_t event) {
  check(g_events.count(event) != 0, "an event that was never made is destroyed");
  g_events[event]++;
  return logged("event-", event, nullptr);
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
  check(g_events.count(event) && g_events[event] == 0, "an event that does not exist is recorded");
  return logged("rec", event, stream);
}
hipError_t hipEventSynchronize(hipEvent_t event) { return logged("sync", event, nullptr); }
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned flags) {
  check(g_events.count(event) && g_events[event] == 0 && flags == 0u, "a stream waits for an event that does not exist");
  return logged("wait", event, stream);
}
hipError_t hipDeviceSynchronize(void) { return logged("drain", nullptr, nullptr); }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { *least = 0; *greatest = -1; return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *stream, unsigned flags, int priority) {
  check(flags == hipStreamNonBlocking && priority == -1, "the side stream is blocking or not at the greatest priority");
  *stream = (hipStream_t)(0x1000u + ++g_handles);
  g_streams[*stream] = 0;
  return logged("stream+", nullptr, *stream);
}
hipError_t hipStreamDestroy(hipStream_t stream) { g_streams[stream]++; return logged("stream-", nullptr, stream); }
hipError_t hipHostMalloc(void **ptr, size_t bytes, unsigned) {
  *ptr = malloc(bytes);
  g_pinned.push_back({*ptr, 0});
  return logged("pinned+", nullptr, nullptr);
}
hipError_t hipHostFree(void *ptr) {
  for (size_t i = g_pinned.size(); i-- > 0;)
    if (g_pinned[i].first == ptr) {
      if (g_pinned[i].second++ == 0) free(ptr);
      return logged("pinned-", nullptr, nullptr);
    }
  check(false, "pinned memory that was never allocated is freed");
  return hipSuccess;
}

int main() {
  one_stream();
  two_streams();
  edits_across_streams();
  edits_on_the_launches_stream();
  ring();
  lifetime();
  if (g_failures) { fprintf(stderr, "scene_sync_check: %d differences\n", g_failures); return 1; }
  printf("scene_sync_check: ok (%zu calls recorded)\n", g_log.size());
  return 0;
}
