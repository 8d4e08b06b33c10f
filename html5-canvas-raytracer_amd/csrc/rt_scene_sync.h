// rt_scene_sync.h — how a resident scene orders its launches, its moves and its texel edits across HIP streams without a host wait, and
// what it owns for that: events, the side stream, two rings of pinned staging.  Nothing of the project is included: every HIP call the
// rules make is in this header, so a plain host compiler can build it against recording fakes (tests/host/scene_sync_check.cpp).
// Methods return hipError_t; callers wrap them in HIP_TRY.  The caller holds the scene's launch_mu around every call.
//
// What exists twice - the camera block, the object block, a launch table - exists for even and odd generations: generation g reads
// copy g & 1, so a move can write the next one, on the scene's own side stream S, while launches with the current one still run.
// Texels live once and an edit is no generation: it is one write on the caller's stream, ordered against the launches around it.
//   OLD[x]    recorded on the caller's stream at the move to generation g (x = (g - 1) & 1): every launch with generations < g precedes
//             it.  The move to g + 1 writes copies (g + 1) & 1 = x only behind it.
//   PREP[b]   recorded on S behind the copies and builds of generation g (b = g & 1): the first launch of g on a stream waits for it.
//   TEXB      recorded on the stream of the launches in flight when an edit's stream is another one: the write waits for it.
//   TEXD      recorded behind an edit's write: the next launch on every OTHER stream waits for it, and so does the next edit on another.
// The rules:
//   R1  Launch on stream X at generation g.  If an edit has happened and its stream is not X, X waits for TEXD, once per (X, edit
//       count).  If PREP[g & 1] has been recorded, X waits for it, once per (X, g).  Then last_stream = X, and several_streams is set
//       if an earlier launch was on another stream.
//   R2  Spread.  When a move or an edit starts while launches are on several streams, no single event covers them: drain the device
//       and forget all launch state and both OLD valid flags.
//   R3  Move to generation G, after R2.  If something was launched since the last move, record OLD[(G - 1) & 1] on last_stream (else
//       the older record still covers them).  If OLD[G & 1] is valid, S waits for it.  Take a ring slot, run the copies and builds on
//       S, record the slot's event on S.  Record PREP[G & 1] on S and clear its list.
//   R4  Edit on stream X, after R2.  If launches are in flight on one stream L other than X, record TEXB on L and X waits for it.  If
//       an earlier edit ran on another stream, X waits for TEXD (two edits may overlap).  Run the write.  Record TEXD on X, bump the
//       edit count and clear the list.
//   R5  Ring.  A slot's 2nd, 3rd, ... use first synchronises on the event of its previous use; the first use waits for nothing.
//   R6  Lazy events.  No event exists before the first move (OLD, PREP) or the first edit (TEXB, TEXD).
#ifndef RT_SCENE_SYNC_H
#define RT_SCENE_SYNC_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

namespace rt_api {

#define RT_SYNC_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// a handle of the runtime (an event, a stream, memory) that is released with its owner: movable, not copyable
template <class T, hipError_t (*RELEASE)(T)> struct owned {
  T h = nullptr;
  owned() = default;
  owned(owned &&o) noexcept : h(o.h) { o.h = nullptr; }
  owned &operator=(owned &&o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
  ~owned() { reset(); }
  void reset() { if (h) (void)RELEASE(h); h = nullptr; }
  explicit operator bool() const { return h != nullptr; }
};
using pinned_mem = owned<void *, hipHostFree>;
// one untimed event, made on first need
struct event : owned<hipEvent_t, hipEventDestroy> {
  hipError_t make() { return h ? hipSuccess : hipEventCreateWithFlags(&h, hipEventDisableTiming); }
};

// Pinned staging for small copies: one allocation of n_slots slots, each guarded by an event recorded behind the copy that read it (R5).
// (16 slots: the host may run eight frames ahead of the GPU in an animation.)
struct pinned_ring {
  static constexpr uint32_t n_slots = 16u;
  struct slot { uint8_t *h = nullptr; event read; bool used = false; };
  slot slots[n_slots];
  pinned_mem pool; uint32_t next = 0;
  hipError_t make(size_t slot_bytes) {
    if (!pool) RT_SYNC_TRY(hipHostMalloc(&pool.h, slot_bytes * n_slots, hipHostMallocDefault));
    for (uint32_t i = 0; i < n_slots; i++) { slots[i].h = (uint8_t *)pool.h + i * slot_bytes; RT_SYNC_TRY(slots[i].read.make()); }
    return hipSuccess;
  }
  // the next slot, free to be written: the copy that read it last has finished (the one host wait, taken n_slots copies ahead of the GPU)
  hipError_t acquire(slot **out) {
    slot &g = slots[next++ % n_slots];
    *out = &g;
    const hipError_t e = g.used ? hipEventSynchronize(g.read.h) : hipSuccess;
    g.used = true;
    return e;
  }
  // the copy that reads the slot has been enqueued on `stream`
  hipError_t done(slot *g, hipStream_t stream) { return hipEventRecord(g->read.h, stream); }
};

// An event other streams come behind, once each: the stream it was last recorded on, a sequence number (a generation, an edit count)
// and the streams that already wait for that sequence.
struct stream_gate {
  event ev; hipStream_t on = nullptr; uint64_t seq = 0; bool valid = false;
  struct waiter { hipStream_t stream; uint64_t seq; };
  std::vector<waiter> waiting;
  hipError_t open(hipStream_t stream, uint64_t s) {
    RT_SYNC_TRY(hipEventRecord(ev.h, stream));
    on = stream; seq = s; valid = true; waiting.clear();
    return hipSuccess;
  }
  hipError_t pass(hipStream_t stream, uint64_t s) {
    if (!valid || stream == on) return hipSuccess;
    for (const waiter &q : waiting) if (q.stream == stream && q.seq == s) return hipSuccess;
    RT_SYNC_TRY(hipStreamWaitEvent(stream, ev.h, 0));
    if (waiting.size() >= 16u) waiting.clear();
    waiting.push_back(waiter{stream, s});
    return hipSuccess;
  }
};

struct scene_sync {
  hipStream_t last_stream = nullptr;     // the stream of the scene's last launch; several: launches of this scene are in flight on more than one
  bool any_launch = false, several_streams = false, launched_since_move = false;
  owned<hipStream_t, hipStreamDestroy> side;   // S: a move's copies and table rebuilds run here, beside the previous generation's launches
  event old_done[2]; bool old_valid[2] = {false, false};
  stream_gate prep[2];                   // (sequence: the generation)
  event tex_before;
  stream_gate tex;                       // TEXD (sequence: edits so far)
  pinned_ring moves;                     // a move's camera block and object block, a launch table's parameters; made at upload
  pinned_ring texels;                    // the host form of a texel edit; made by the first one

  // R1, first half: a launch about to be enqueued on `stream` comes behind the last edit and behind generation gen's preparation
  hipError_t before_launch(hipStream_t stream, uint64_t gen) {
    RT_SYNC_TRY(tex.pass(stream, tex.seq));
    return prep[gen & 1u].pass(stream, gen);
  }
  // R1, second half: a launch is enqueued on `stream`: what the next move or edit orders itself behind
  void note_launch(hipStream_t stream) {
    if (any_launch && last_stream != stream) several_streams = true;
    last_stream = stream; any_launch = true; launched_since_move = true;
  }
  // R2 (rare)
  hipError_t drain_if_spread() {
    if (!(any_launch && several_streams)) return hipSuccess;
    RT_SYNC_TRY(hipDeviceSynchronize());
    any_launch = several_streams = launched_since_move = old_valid[0] = old_valid[1] = false;
    return hipSuccess;
  }
  // S (HIGH priority: its few hundred waves are launched INTO a chip the previous frame's trace keeps full; at normal priority the
  // table build's workgroups waited for slots and took 77 us instead of 20, profiles/r04_ab_log.md) and the moves' events (R6)
  hipError_t ensure_side() {
    if (side) return hipSuccess;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    RT_SYNC_TRY(hipStreamCreateWithPriority(&side.h, hipStreamNonBlocking, prio_hi));
    for (int b = 0; b < 2; b++) { RT_SYNC_TRY(old_done[b].make()); RT_SYNC_TRY(prep[b].ev.make()); }
    return hipSuccess;
  }
  // R3 up to S's wait; ensure_side has run
  hipError_t begin_generation(uint64_t G) {
    RT_SYNC_TRY(drain_if_spread());
    if (launched_since_move && any_launch) { RT_SYNC_TRY(hipEventRecord(old_done[(G - 1u) & 1u].h, last_stream)); old_valid[(G - 1u) & 1u] = true; }
    launched_since_move = false;
    return old_valid[G & 1u] ? hipStreamWaitEvent(side.h, old_done[G & 1u].h, 0) : hipSuccess;
  }
  hipError_t end_generation(uint64_t G) { return prep[G & 1u].open(side.h, G); }
  // R4 in front of the write ...
  hipError_t begin_edit(hipStream_t stream) {
    RT_SYNC_TRY(tex_before.make()); RT_SYNC_TRY(tex.ev.make());
    if (any_launch && several_streams) RT_SYNC_TRY(drain_if_spread());
    else if (any_launch && last_stream != stream) { RT_SYNC_TRY(hipEventRecord(tex_before.h, last_stream)); RT_SYNC_TRY(hipStreamWaitEvent(stream, tex_before.h, 0)); }
    return tex.valid && tex.on != stream ? hipStreamWaitEvent(stream, tex.ev.h, 0) : hipSuccess;
  }
  // ... and behind it (also behind the pieces of a write that failed half way)
  hipError_t end_edit(hipStream_t stream) { return tex.open(stream, tex.seq + 1u); }
};

#undef RT_SYNC_TRY

}  // namespace rt_api

#endif
