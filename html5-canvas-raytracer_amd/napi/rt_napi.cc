// rt_napi.cc — thin N-API shim between the Node.js host (js/index.js) and the C ABI of
// include/rt_hip.h.  It does no rendering and no scene logic: the scene arrives already flattened
// (js/flatten.js) as one ArrayBuffer, and the frame goes back as a Uint8ClampedArray over the
// pinned host buffer the library filled — the object the reference's ImageData.data is
// (main.js:83), so `context.putImageData(new ImageData(data, w, h), 0, 0)` works unchanged.
//
// Exports:  init(maxDevices) -> deviceCount      render(blob, w, h, flags) -> {data, width, height, stats}
//           renderAsync(blob, w, h, flags) -> Promise of the same        shutdown()      abiVersion()
//           renderAdaptive(blob, w, h, flags, k, threshold[, into[, async]]) -> the same (or a Promise of it), stats.refined added:
//           adaptive supersampling (rt_render_adaptive)
//           renderProgressive(blob, w, h, flags, bands, onBand(firstRow, nRows)) -> {data, promise}: `data` is the frame
//           being filled; onBand fires on the main thread as each row band lands in it; the promise resolves to the stats
//           renderHits(blob, w, h, wantDepth, wantNormal) -> {id: Int32Array, depth: Float64Array | null, normal: Float32Array | null}
//           pick(blob, w, h, sx, sy) -> {index, inside, t, point, normal, u, v} or null (a miss); sx, sy in sample-grid coordinates
//           traceRays(blob, rays: Float64Array (6 per ray), segs, wantRgb, wantRgba, wantHits, bin) -> {rgb: Float64Array | null,
//           rgba: Uint8ClampedArray | null, hits: Array of pick's records (null = a miss) | null}: intersectWorld per ray (rt_trace_rays;
//           bin: rt_trace_rays_binned, the list ordered on the GPU first - the same results; two more booleans, wavefront and
//           orderLevels: rt_trace_rays_wavefront, the same rgb and rgba level by level, plus levelCounts; six more, levels and lighting's tail
//           offs, nSamples, stride, base, lightRadius: rt_trace_rays_soft, the wavefront form with the first `levels` levels' nodes relit;
//           one more boolean, recursive: rt_trace_rays_soft_recursive, the same bytes from one launch per chunk)
//           shadeRays(blob, rays, pix: Uint32Array | null, path: Uint32Array | null, bin) -> {nodes: ArrayBuffer of rt_node records, count}
//           relightRays(blob, rays, pix, path, bin, offs, nSamples, stride, base, lightRadius) -> the same, with soft lights (rt_relight_rays)
//           traceView(blob, view: Uint8Array (the 136 bytes of rt_view, table pointers ignored), lon: Float64Array | null, lat: Float64Array | null,
//           w, h, segs, wantRgb, wantRgba, wantHits) -> traceRays' result for the view's w x h rays, generated on the GPU (rt_trace_view;
//           six more, levels and lighting's tail: rt_trace_view_soft, the soft trace of the view in one launch per chunk of rows, no hits)
//           equirectTables(w, h) -> {lon: Float64Array (2 w), lat: Float64Array (2 h)} (rt_view_equirect_tables)
//           viewSamplesGrid(k) -> Float64Array (dx, dy, lu, lv per sample: rt_view_samples_grid)
//           equirectSampleTables(w, h, samples) -> {lon, lat}: one table per sample (rt_view_equirect_sample_tables)
//           traceViewSamples(blob, view, lon, lat, w, h, samples: Float64Array (4 per sample), lens: Float64Array (radius, focus) | null, segs,
//           wantRgb, wantRgba) -> {rgb, rgba, hits: null, kernel_ms}: the mean of one trace per sample (rt_trace_view_samples)
//           (these, and renderAdaptive, are not enumerable: the enumerable surface is the frame API of the first revision)
// Every failure of the library becomes a thrown JS Error carrying rt_last_error().
//
// Build: g++ -shared -fPIC -I/usr/include/node rt_napi.cc -L../csrc -lrt_hip  (napi/Makefile; no node-gyp).

#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/rt_hip.h"

namespace {

#define NAPI_TRY(call)                                                        \
  do {                                                                        \
    if ((call) != napi_ok) {                                                  \
      napi_throw_error(env, nullptr, "N-API call failed: " #call);            \
      return nullptr;                                                         \
    }                                                                         \
  } while (0)

napi_value throw_rt(napi_env env, const char *what, int rc) {
  std::string msg = std::string(what) + " failed (" + std::to_string(rc) + "): " + rt_last_error();
  napi_throw_error(env, rc == RT_ERR_UNSUPPORTED ? "RT_ERR_UNSUPPORTED" : rc == RT_ERR_DEVICE ? "RT_ERR_DEVICE" : "RT_ERR", msg.c_str());
  return nullptr;
}

void free_pinned(napi_env, void *data, void *) { rt_free_pinned(data); }

struct args {
  void *blob = nullptr;      // the scene blob; `owned` when it is our (re-aligned / off-thread) copy
  bool owned = false;
  size_t bytes = 0;
  uint32_t w = 0, h = 0, flags = 0;
  uint32_t k = 0, threshold = 0;   // renderAdaptive: k x k samples where the frame has edges (k == 0: a plain render)
  uint64_t refined = 0;
  uint8_t *out = nullptr;
  rt_stats st{};
  int rc = 0;
  std::string err;
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
};

bool parse(napi_env env, napi_callback_info info, args *a, bool copy_blob) {
  size_t argc = 4;
  napi_value argv[4];
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3) {
    napi_throw_type_error(env, nullptr, "render(blob: ArrayBuffer, width, height[, flags])");
    return false;
  }
  bool is_ab = false;
  napi_is_arraybuffer(env, argv[0], &is_ab);
  void *data = nullptr;
  size_t len = 0;
  if (is_ab) napi_get_arraybuffer_info(env, argv[0], &data, &len);
  else {
    bool is_ta = false;
    napi_is_typedarray(env, argv[0], &is_ta);
    if (!is_ta) { napi_throw_type_error(env, nullptr, "scene blob must be an ArrayBuffer or a typed array"); return false; }
    napi_typedarray_type t; napi_value ab; size_t off;
    napi_get_typedarray_info(env, argv[0], &t, &len, &data, &ab, &off);
    if (t != napi_uint8_array && t != napi_uint8_clamped_array) { napi_throw_type_error(env, nullptr, "typed-array blob must be Uint8Array"); return false; }
  }
  if (napi_get_value_uint32(env, argv[1], &a->w) != napi_ok || napi_get_value_uint32(env, argv[2], &a->h) != napi_ok || a->w == 0 || a->h == 0) {
    napi_throw_type_error(env, nullptr, "width and height must be positive integers");
    return false;
  }
  if (argc >= 4) napi_get_value_uint32(env, argv[3], &a->flags);
  a->bytes = len;
  if (copy_blob || ((uintptr_t)data & 7u) != 0) {       // the library wants 8-byte alignment
    a->blob = aligned_alloc(16, (len + 15) & ~(size_t)15);
    if (!a->blob) { napi_throw_error(env, nullptr, "out of memory"); return false; }
    memcpy(a->blob, data, len);
    a->owned = true;
  } else a->blob = data;
  return true;
}

// `into`: the caller's own frame (render(..., {into})), handed back as `data`; else a new typed array over the pinned frame
napi_value make_result(napi_env env, args *a, napi_value into = nullptr) {
  const size_t n = (size_t)a->w * a->h * 4u;
  napi_value ab, ta = into, res, stats, v;
  if (!into) {
    NAPI_TRY(napi_create_external_arraybuffer(env, a->out, n, free_pinned, nullptr, &ab));
    a->out = nullptr;    // owned by the ArrayBuffer's finalizer from here on
    NAPI_TRY(napi_create_typedarray(env, napi_uint8_clamped_array, n, ab, 0, &ta));
  }
  NAPI_TRY(napi_create_object(env, &res));
  NAPI_TRY(napi_create_object(env, &stats));
  napi_set_named_property(env, res, "data", ta);
  napi_create_uint32(env, a->w, &v); napi_set_named_property(env, res, "width", v);
  napi_create_uint32(env, a->h, &v); napi_set_named_property(env, res, "height", v);
  napi_create_double(env, a->st.kernel_ms, &v); napi_set_named_property(env, stats, "kernel_ms", v);
  napi_create_double(env, a->st.total_ms, &v); napi_set_named_property(env, stats, "total_ms", v);
  napi_create_double(env, (double)a->st.pixels, &v); napi_set_named_property(env, stats, "pixels", v);
  napi_create_double(env, (double)a->st.rays, &v); napi_set_named_property(env, stats, "rays", v);
  napi_create_double(env, (double)a->st.shadow_rays, &v); napi_set_named_property(env, stats, "shadow_rays", v);
  napi_create_double(env, (double)a->st.sphere_tests, &v); napi_set_named_property(env, stats, "sphere_tests", v);
  napi_create_double(env, (double)a->st.exact_samples, &v); napi_set_named_property(env, stats, "exact_samples", v);
  if (a->k) { napi_create_double(env, (double)a->refined, &v); napi_set_named_property(env, stats, "refined", v); }
  { char rep[96]; napi_value sv; if (rt_elapsed_report(&a->st, rep, sizeof rep) > 0) { napi_create_string_utf8(env, rep, NAPI_AUTO_LENGTH, &sv); napi_set_named_property(env, stats, "report", sv); }
    napi_create_string_utf8(env, rt_build_id(), NAPI_AUTO_LENGTH, &sv); napi_set_named_property(env, stats, "build", sv); }
  napi_set_named_property(env, res, "stats", stats);
  return res;
}

napi_value Init(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  uint32_t maxdev = 0;
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  if (argc >= 1) napi_get_value_uint32(env, argv[0], &maxdev);
  int rc = rt_init((int)maxdev);
  if (rc != RT_OK) return throw_rt(env, "rt_init", rc);
  napi_value v;
  napi_create_int32(env, rt_device_count(), &v);
  return v;
}

// render(blob, width, height[, flags[, into]]).  `into`: a Uint8ClampedArray / Uint8Array of 4*width*height bytes that receives the
// frame - the reference creates its ImageData once (main.js:83) and every redraw fills it again (main.js:195-200).  A frame that an
// earlier render() returned is pinned memory the GPU stores into directly; any other array is pageable memory (slower, same bytes).
napi_value Render(napi_env env, napi_callback_info info) {
  args a;
  if (!parse(env, info, &a, false)) return nullptr;
  napi_value res = nullptr;
  {
    size_t argc = 5;
    napi_value argv[5];
    napi_valuetype t = napi_undefined;
    napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
    if (argc >= 5) napi_typeof(env, argv[4], &t);
    if (argc >= 5 && t != napi_undefined && t != napi_null) {
      bool is_ta = false;
      napi_is_typedarray(env, argv[4], &is_ta);
      napi_typedarray_type tt = napi_int8_array; size_t len = 0, off = 0; void *data = nullptr; napi_value ab;
      if (is_ta) napi_get_typedarray_info(env, argv[4], &tt, &len, &data, &ab, &off);
      if (!is_ta || (tt != napi_uint8_array && tt != napi_uint8_clamped_array) || len != (size_t)a.w * a.h * 4u || !data) {
        if (a.owned) free(a.blob);
        napi_throw_type_error(env, nullptr, "into must be a Uint8ClampedArray / Uint8Array of 4*width*height bytes");
        return nullptr;
      }
      a.rc = rt_render(a.blob, a.bytes, a.w, a.h, (uint8_t *)data, a.flags, &a.st);
      res = (a.rc != RT_OK) ? throw_rt(env, "rt_render", a.rc) : make_result(env, &a, argv[4]);
      if (a.owned) free(a.blob);
      return res;
    }
  }
  a.out = (uint8_t *)rt_alloc_pinned((size_t)a.w * a.h * 4u);
  if (!a.out) res = throw_rt(env, "rt_alloc_pinned", RT_ERR_NOMEM);
  else {
    a.rc = rt_render(a.blob, a.bytes, a.w, a.h, a.out, a.flags, &a.st);
    if (a.rc != RT_OK) { rt_free_pinned(a.out); a.out = nullptr; res = throw_rt(env, "rt_render", a.rc); }
    else res = make_result(env, &a);
  }
  if (a.owned) free(a.blob);
  return res;
}

void exec_async(napi_env, void *p) {
  args *a = (args *)p;
  a->out = (uint8_t *)rt_alloc_pinned((size_t)a->w * a->h * 4u);
  if (!a->out) { a->rc = RT_ERR_NOMEM; a->err = rt_last_error(); return; }
  a->rc = a->k ? rt_render_adaptive(a->blob, a->bytes, a->w, a->h, a->k, a->threshold, a->out, nullptr, a->flags, &a->st, &a->refined)
               : rt_render(a->blob, a->bytes, a->w, a->h, a->out, a->flags, &a->st);
  if (a->rc != RT_OK) { a->err = rt_last_error(); rt_free_pinned(a->out); a->out = nullptr; }   // rt_last_error is per thread: read it here
}

void done_async(napi_env env, napi_status, void *p) {
  args *a = (args *)p;
  if (a->rc == RT_OK) {
    napi_value res = make_result(env, a);
    if (res) napi_resolve_deferred(env, a->deferred, res);
  } else {
    napi_value msg, err;
    std::string m = std::string(a->k ? "rt_render_adaptive" : "rt_render") + " failed (" + std::to_string(a->rc) + "): " + a->err;
    napi_create_string_utf8(env, m.c_str(), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, nullptr, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  }
  napi_delete_async_work(env, a->work);
  if (a->owned) free(a->blob);
  delete a;
}

napi_value RenderAsync(napi_env env, napi_callback_info info) {
  args *a = new args();
  if (!parse(env, info, a, true)) { if (a->owned) free(a->blob); delete a; return nullptr; }
  napi_value promise, name;
  NAPI_TRY(napi_create_promise(env, &a->deferred, &promise));
  napi_create_string_utf8(env, "rt_render", NAPI_AUTO_LENGTH, &name);
  NAPI_TRY(napi_create_async_work(env, nullptr, name, exec_async, done_async, a, &a->work));
  NAPI_TRY(napi_queue_async_work(env, a->work));
  return promise;
}

// renderAdaptive(blob, width, height, flags, k, threshold[, into[, async]]): the supersample-1 frame with k x k samples (k 2..4) for
// the pixels that differ from a 4-neighbour by `threshold` (0..256) or more (rt_render_adaptive); stats.refined is how many there were.
// `into` as for render; async === true: a Promise of the same result, the work off the event loop (no `into` then).
napi_value RenderAdaptive(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  napi_valuetype t = napi_undefined;
  bool async = false;
  uint32_t k = 0, threshold = 0;
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  if (argc < 6 || napi_get_value_uint32(env, argv[4], &k) != napi_ok || napi_get_value_uint32(env, argv[5], &threshold) != napi_ok || k == 0) {
    napi_throw_type_error(env, nullptr, "renderAdaptive(blob, width, height, flags, k, threshold[, into[, async]])");
    return nullptr;
  }
  if (argc >= 8) napi_get_value_bool(env, argv[7], &async);
  if (argc >= 7) napi_typeof(env, argv[6], &t);
  const bool have_into = argc >= 7 && t != napi_undefined && t != napi_null;
  args *a = new args();
  if (!parse(env, info, a, async)) { if (a->owned) free(a->blob); delete a; return nullptr; }
  a->k = k; a->threshold = threshold;
  if (async) {
    napi_value promise, name;
    if (have_into) { if (a->owned) free(a->blob); delete a; napi_throw_type_error(env, nullptr, "renderAdaptive: no `into` with async"); return nullptr; }
    NAPI_TRY(napi_create_promise(env, &a->deferred, &promise));
    napi_create_string_utf8(env, "rt_render_adaptive", NAPI_AUTO_LENGTH, &name);
    NAPI_TRY(napi_create_async_work(env, nullptr, name, exec_async, done_async, a, &a->work));
    NAPI_TRY(napi_queue_async_work(env, a->work));
    return promise;
  }
  napi_value res = nullptr;
  uint8_t *dst = nullptr;
  if (have_into) {
    bool is_ta = false;
    napi_is_typedarray(env, argv[6], &is_ta);
    napi_typedarray_type tt = napi_int8_array; size_t len = 0, off = 0; void *data = nullptr; napi_value ab;
    if (is_ta) napi_get_typedarray_info(env, argv[6], &tt, &len, &data, &ab, &off);
    if (!is_ta || (tt != napi_uint8_array && tt != napi_uint8_clamped_array) || len != (size_t)a->w * a->h * 4u || !data)
      napi_throw_type_error(env, nullptr, "into must be a Uint8ClampedArray / Uint8Array of 4*width*height bytes");
    else dst = (uint8_t *)data;
  } else {
    dst = a->out = (uint8_t *)rt_alloc_pinned((size_t)a->w * a->h * 4u);
    if (!dst) throw_rt(env, "rt_alloc_pinned", RT_ERR_NOMEM);
  }
  if (dst) {
    a->rc = rt_render_adaptive(a->blob, a->bytes, a->w, a->h, a->k, a->threshold, dst, nullptr, a->flags, &a->st, &a->refined);
    if (a->rc != RT_OK) { if (a->out) rt_free_pinned(a->out); a->out = nullptr; res = throw_rt(env, "rt_render_adaptive", a->rc); }
    else res = make_result(env, a, have_into ? argv[6] : nullptr);
  }
  if (a->owned) free(a->blob);
  delete a;
  return res;
}

// ---- progressive delivery: the frame buffer exists from the start (the page can keep a view of it), bands are announced
//      from the worker thread through a thread-safe function, the promise resolves when the frame is whole ----
struct prog_args : args {
  uint32_t bands = 4;
  napi_threadsafe_function tsfn = nullptr;
};
struct band_note { uint32_t row0, rows; };

void prog_call_js(napi_env env, napi_value js_cb, void *, void *data) {
  band_note *b = (band_note *)data;
  if (env && js_cb) {
    napi_value undef, argv[2];
    napi_get_undefined(env, &undef);
    napi_create_uint32(env, b->row0, &argv[0]);
    napi_create_uint32(env, b->rows, &argv[1]);
    napi_call_function(env, undef, js_cb, 2, argv, nullptr);
  }
  delete b;
}

void prog_on_band(void *user, uint32_t row0, uint32_t rows) {
  prog_args *a = (prog_args *)user;
  napi_call_threadsafe_function(a->tsfn, new band_note{row0, rows}, napi_tsfn_blocking);
}

void prog_exec(napi_env, void *p) {
  prog_args *a = (prog_args *)p;
  a->rc = rt_render_progressive(a->blob, a->bytes, a->w, a->h, a->out, a->bands, prog_on_band, a, a->flags, &a->st);
  if (a->rc != RT_OK) a->err = rt_last_error();
}

// The band notes travel through the thread-safe function's queue; the async work's completion callback may overtake the
// last of them.  So the work's completion only RELEASES the function, and the promise is settled in the function's
// finalizer, which runs on the main thread after the queue has drained: every onBand has fired before the promise resolves.
void prog_done(napi_env env, napi_status, void *p) {
  prog_args *a = (prog_args *)p;
  napi_delete_async_work(env, a->work);
  napi_release_threadsafe_function(a->tsfn, napi_tsfn_release);
}

void prog_finalize(napi_env env, void *data, void *) {
  prog_args *a = (prog_args *)data;
  if (a->rc == RT_OK) {
    napi_value stats, v;
    napi_create_object(env, &stats);
    napi_create_double(env, a->st.kernel_ms, &v); napi_set_named_property(env, stats, "kernel_ms", v);
    napi_create_double(env, a->st.total_ms, &v); napi_set_named_property(env, stats, "total_ms", v);
    napi_create_double(env, (double)a->st.pixels, &v); napi_set_named_property(env, stats, "pixels", v);
    { char rep[96]; napi_value sv; if (rt_elapsed_report(&a->st, rep, sizeof rep) > 0) { napi_create_string_utf8(env, rep, NAPI_AUTO_LENGTH, &sv); napi_set_named_property(env, stats, "report", sv); }
      napi_create_string_utf8(env, rt_build_id(), NAPI_AUTO_LENGTH, &sv); napi_set_named_property(env, stats, "build", sv); }
    napi_resolve_deferred(env, a->deferred, stats);
  } else {
    napi_value msg, err;
    std::string m = "rt_render_progressive failed (" + std::to_string(a->rc) + "): " + a->err;
    napi_create_string_utf8(env, m.c_str(), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, nullptr, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
  }
  if (a->owned) free(a->blob);
  delete a;
}

napi_value RenderProgressive(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  napi_valuetype t = napi_undefined;
  if (argc >= 6) napi_typeof(env, argv[5], &t);
  if (argc < 6 || t != napi_function) { napi_throw_type_error(env, nullptr, "renderProgressive(blob, width, height, flags, bands, onBand)"); return nullptr; }
  prog_args *a = new prog_args();
  if (!parse(env, info, a, true)) { if (a->owned) free(a->blob); delete a; return nullptr; }
  napi_get_value_uint32(env, argv[4], &a->bands);
  const size_t n = (size_t)a->w * a->h * 4u;
  a->out = (uint8_t *)rt_alloc_pinned(n);
  if (!a->out) { if (a->owned) free(a->blob); delete a; return throw_rt(env, "rt_alloc_pinned", RT_ERR_NOMEM); }
  napi_value ab, ta, res, promise, name;
  // from here on the pinned frame belongs to the ArrayBuffer (freed by its finalizer, whatever happens to the render)
  if (napi_create_external_arraybuffer(env, a->out, n, free_pinned, nullptr, &ab) != napi_ok) {
    rt_free_pinned(a->out); if (a->owned) free(a->blob); delete a;
    napi_throw_error(env, nullptr, "napi_create_external_arraybuffer failed");
    return nullptr;
  }
  NAPI_TRY(napi_create_typedarray(env, napi_uint8_clamped_array, n, ab, 0, &ta));
  NAPI_TRY(napi_create_promise(env, &a->deferred, &promise));
  napi_create_string_utf8(env, "rt_render_progressive", NAPI_AUTO_LENGTH, &name);
  NAPI_TRY(napi_create_threadsafe_function(env, argv[5], nullptr, name, 0, 1, a, prog_finalize, nullptr, prog_call_js, &a->tsfn));
  NAPI_TRY(napi_create_async_work(env, nullptr, name, prog_exec, prog_done, a, &a->work));
  NAPI_TRY(napi_queue_async_work(env, a->work));
  NAPI_TRY(napi_create_object(env, &res));
  napi_set_named_property(env, res, "data", ta);
  napi_set_named_property(env, res, "promise", promise);
  return res;
}

napi_value Shutdown(napi_env, napi_callback_info) { rt_shutdown(); return nullptr; }

// main.js:3 / :204-205: the build stamp and the end-of-frame report 'build #<id> (<elapsed>ms)'
napi_value BuildId(napi_env env, napi_callback_info) {
  napi_value v;
  napi_create_string_utf8(env, rt_build_id(), NAPI_AUTO_LENGTH, &v);
  return v;
}

napi_value AbiVersion(napi_env env, napi_callback_info) {
  napi_value v;
  napi_create_uint32(env, rt_abi_version(), &v);
  return v;
}

napi_value Validate(napi_env env, napi_callback_info info) {
  args a;
  size_t argc = 1; napi_value argv[1]; void *data = nullptr; size_t len = 0; bool is_ab = false;
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  if (argc < 1 || napi_is_arraybuffer(env, argv[0], &is_ab) != napi_ok || !is_ab) { napi_throw_type_error(env, nullptr, "validate(blob: ArrayBuffer)"); return nullptr; }
  napi_get_arraybuffer_info(env, argv[0], &data, &len);
  void *copy = aligned_alloc(16, (len + 15) & ~(size_t)15);
  memcpy(copy, data, len);
  const int rc = rt_scene_validate(copy, len);
  free(copy);
  if (rc != RT_OK) return throw_rt(env, "rt_scene_validate", rc);
  napi_value v; napi_get_boolean(env, true, &v);
  return v;
}

// renderHits(blob, w, h, wantDepth, wantNormal): the primary hit of every sample (rt_render_hits) into typed arrays the JS heap owns
napi_value RenderHits(napi_env env, napi_callback_info info) {
  args a;
  if (!parse(env, info, &a, false)) return nullptr;
  size_t argc = 5;
  napi_value argv[5];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool want_depth = true, want_normal = true;
  if (argc >= 4) napi_get_value_bool(env, argv[3], &want_depth);
  if (argc >= 5) napi_get_value_bool(env, argv[4], &want_normal);
  // the sample grid's size comes from the blob: a malformed one is refused before anything is allocated
  const int vrc = rt_scene_validate(a.blob, a.bytes);
  const uint32_t k = vrc == RT_OK ? ((const rt_scene_header *)a.blob)->supersample : 1u;
  const size_t n = (size_t)k * a.w * k * a.h;
  napi_value ab_id = nullptr, ab_depth = nullptr, ab_normal = nullptr, res, v;
  void *p_id = nullptr, *p_depth = nullptr, *p_normal = nullptr;
  const bool ok = vrc == RT_OK && a.w <= 65536u && a.h <= 65536u && n < (1ull << 32) &&
                  napi_create_arraybuffer(env, n * 4u, &p_id, &ab_id) == napi_ok &&
                  (!want_depth || napi_create_arraybuffer(env, n * 8u, &p_depth, &ab_depth) == napi_ok) &&
                  (!want_normal || napi_create_arraybuffer(env, n * 12u, &p_normal, &ab_normal) == napi_ok);
  if (!ok) {
    if (a.owned) free(a.blob);
    if (vrc != RT_OK) return throw_rt(env, "rt_render_hits", vrc);
    napi_throw_error(env, nullptr, "renderHits: the frame is too large or its output arrays cannot be allocated");
    return nullptr;
  }
  const rt_hit_buffers b = {(int32_t *)p_id, (double *)p_depth, (float *)p_normal};
  a.rc = rt_render_hits(a.blob, a.bytes, a.w, a.h, &b, &a.st);
  if (a.owned) free(a.blob);
  if (a.rc != RT_OK) return throw_rt(env, "rt_render_hits", a.rc);
  NAPI_TRY(napi_create_object(env, &res));
  NAPI_TRY(napi_create_typedarray(env, napi_int32_array, n, ab_id, 0, &v)); napi_set_named_property(env, res, "id", v);
  if (want_depth) { NAPI_TRY(napi_create_typedarray(env, napi_float64_array, n, ab_depth, 0, &v)); } else napi_get_null(env, &v);
  napi_set_named_property(env, res, "depth", v);
  if (want_normal) { NAPI_TRY(napi_create_typedarray(env, napi_float32_array, 3 * n, ab_normal, 0, &v)); } else napi_get_null(env, &v);
  napi_set_named_property(env, res, "normal", v);
  napi_create_uint32(env, k * a.w, &v); napi_set_named_property(env, res, "width", v);
  napi_create_uint32(env, k * a.h, &v); napi_set_named_property(env, res, "height", v);
  napi_create_double(env, a.st.kernel_ms, &v); napi_set_named_property(env, res, "kernel_ms", v);
  return res;
}

napi_value doubles(napi_env env, const double *x, int n) {
  napi_value arr, v;
  napi_create_array_with_length(env, n, &arr);
  for (int i = 0; i < n; i++) { napi_create_double(env, x[i], &v); napi_set_element(env, arr, i, v); }
  return arr;
}

// a hit record as pick and traceRays return it: {index, inside, t, point, normal, u, v}, or null on a miss
napi_value hit_object(napi_env env, const rt_hit &r) {
  napi_value res, v;
  if (r.object < 0) { napi_get_null(env, &res); return res; }
  NAPI_TRY(napi_create_object(env, &res));
  napi_create_int32(env, r.object, &v); napi_set_named_property(env, res, "index", v);
  napi_get_boolean(env, r.inside != 0, &v); napi_set_named_property(env, res, "inside", v);
  napi_create_double(env, r.t, &v); napi_set_named_property(env, res, "t", v);
  napi_set_named_property(env, res, "point", doubles(env, r.point, 3));
  napi_set_named_property(env, res, "normal", doubles(env, r.normal, 3));
  napi_create_double(env, r.u, &v); napi_set_named_property(env, res, "u", v);
  napi_create_double(env, r.v, &v); napi_set_named_property(env, res, "v", v);
  return res;
}

// pick(blob, w, h, sx, sy): one sample's hit record (rt_pick), or null on a miss
napi_value Pick(napi_env env, napi_callback_info info) {
  args a;
  if (!parse(env, info, &a, false)) return nullptr;
  size_t argc = 5;
  napi_value argv[5];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  uint32_t xy[2];
  if (argc < 5 || napi_get_value_uint32(env, argv[3], &xy[0]) != napi_ok || napi_get_value_uint32(env, argv[4], &xy[1]) != napi_ok) {
    if (a.owned) free(a.blob);
    napi_throw_type_error(env, nullptr, "pick(blob, width, height, sx, sy): sx, sy must be non-negative integers");
    return nullptr;
  }
  rt_hit r;
  a.rc = rt_pick(a.blob, a.bytes, a.w, a.h, 1u, xy, &r);
  if (a.owned) free(a.blob);
  if (a.rc != RT_OK) return throw_rt(env, "rt_pick", a.rc);
  return hit_object(env, r);
}

// (defined with the sampled lights below; traceRays' soft tail and relightRays take the same five arguments)
bool lighting_args(napi_env env, size_t argc, napi_value *argv, size_t at, const char *who, struct rt_lighting *a, const double **offs, bool want[4]);

napi_value TraceRays(napi_env env, napi_callback_info info) {
  size_t argc = 16;
  napi_value argv[16];
  bool is_ta = false, is_rays = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_rays) != napi_ok || !is_rays) {
    napi_throw_type_error(env, nullptr, "traceRays(blob: Uint8Array, rays: Float64Array[, segs, wantRgb, wantRgba, wantHits, bin, wavefront, orderLevels, levels, offs, nSamples, stride, base, lightRadius, recursive])");
    return nullptr;
  }
  napi_typedarray_type bt, rt; napi_value ab; size_t off, blob_len = 0, ray_len = 0;
  void *blob_data = nullptr, *ray_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &rt, &ray_len, &ray_data, &ab, &off);
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || rt != napi_float64_array || ray_len == 0 || ray_len % 6u != 0) {
    napi_throw_type_error(env, nullptr, "traceRays: the blob must be a Uint8Array and the rays a non-empty Float64Array of 6 numbers per ray");
    return nullptr;
  }
  uint32_t segs = 0;
  bool want[3] = {true, false, false};
  if (argc >= 3) napi_get_value_uint32(env, argv[2], &segs);
  for (size_t i = 0; i < 3 && 3 + i < argc; i++) napi_get_value_bool(env, argv[3 + i], &want[i]);
  bool bin = false;                                     // rt_trace_rays_binned: the GPU orders each chunk before it traces it
  if (argc >= 7) napi_get_value_bool(env, argv[6], &bin);
  bool wavefront = false, order_levels = false;         // rt_trace_rays_wavefront: level by level through shade, spawn and fold - the same bytes
  if (argc >= 8) napi_get_value_bool(env, argv[7], &wavefront);
  if (argc >= 9) napi_get_value_bool(env, argv[8], &order_levels);
  // soft lights (rt_trace_rays_soft): levels, then the tail lighting takes - offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius
  // ... and `recursive`: the soft trace in one launch per chunk (rt_trace_rays_soft_recursive) instead of the wavefront loop - the same bytes
  bool soft = false, recursive = false;
  uint32_t levels = 0;
  struct rt_lighting la;
  const double *offs = nullptr;
  if (argc > 9) {
    napi_valuetype vt;
    napi_typeof(env, argv[9], &vt);
    soft = vt != napi_undefined && vt != napi_null;
  }
  if (soft) {
    const char *who = "traceRays: soft lights are levels, offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius";
    bool unused[4];
    if (napi_get_value_uint32(env, argv[9], &levels) != napi_ok) {
      napi_throw_type_error(env, nullptr, who);
      return nullptr;
    }
    if (!lighting_args(env, argc, argv, 10, who, &la, &offs, unused)) return nullptr;
    if (argc > 15) napi_get_value_bool(env, argv[15], &recursive);
    wavefront = !recursive;                             // (the wavefront loop with a relight behind the shade of the first `levels` levels)
    if (recursive && (want[2] || order_levels)) {
      napi_throw_type_error(env, nullptr, "traceRays: the recursive soft trace returns no hit records and has no levels to order");
      return nullptr;
    }
  }
  if (wavefront && (want[2] || bin)) {
    napi_throw_type_error(env, nullptr, "traceRays: the wavefront form returns no hit records and takes the first level in the list's order");
    return nullptr;
  }
  const size_t n = ray_len / 6u;
  // the library wants the blob 8-byte and the rays 16-byte aligned: one aligned copy holds both
  const size_t blob_room = (blob_len + 15) & ~(size_t)15;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + ((n * 48u + 15) & ~(size_t)15));
  napi_value ab_rgb = nullptr, ab_rgba = nullptr, res, v;
  void *p_rgb = nullptr, *p_rgba = nullptr;
  rt_hit *hits = want[2] ? (rt_hit *)malloc(n * sizeof(rt_hit)) : nullptr;
  if (!mem || (want[2] && !hits) || (want[0] && napi_create_arraybuffer(env, n * 24u, &p_rgb, &ab_rgb) != napi_ok) ||
      (want[1] && napi_create_arraybuffer(env, n * 4u, &p_rgba, &ab_rgba) != napi_ok)) {
    free(mem); free(hits);
    napi_throw_error(env, nullptr, "traceRays: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  memcpy(mem + blob_room, ray_data, n * 48u);
  const rt_ray_outputs out = {(double *)p_rgb, (uint8_t *)p_rgba, hits};
  rt_stats st;
  uint64_t level_counts[RT_MAX_SEGS] = {0};
  const int rc = recursive ? rt_trace_rays_soft_recursive(mem, blob_len, &la, offs, levels, n, (const double *)(mem + blob_room), segs, bin ? 1 : 0, &out, &st)
                 : soft ? rt_trace_rays_soft(mem, blob_len, &la, offs, levels, n, (const double *)(mem + blob_room), segs, order_levels ? 1 : 0, &out, &st, level_counts)
                 : wavefront ? rt_trace_rays_wavefront(mem, blob_len, n, (const double *)(mem + blob_room), segs, order_levels ? 1 : 0, &out, &st, level_counts)
                             : (bin ? rt_trace_rays_binned : rt_trace_rays)(mem, blob_len, n, (const double *)(mem + blob_room), segs, &out, &st);
  free(mem);
  if (rc != RT_OK) { free(hits); return throw_rt(env, recursive ? "rt_trace_rays_soft_recursive" : soft ? "rt_trace_rays_soft" : wavefront ? "rt_trace_rays_wavefront" : bin ? "rt_trace_rays_binned" : "rt_trace_rays", rc); }
  napi_create_object(env, &res);
  if (wavefront) {                                      // the rays shaded per level
    napi_value lc, c;
    napi_create_array_with_length(env, RT_MAX_SEGS, &lc);
    for (uint32_t i = 0; i < RT_MAX_SEGS; i++) { napi_create_double(env, (double)level_counts[i], &c); napi_set_element(env, lc, i, c); }
    napi_set_named_property(env, res, "levelCounts", lc);
  }
  if (want[0]) napi_create_typedarray(env, napi_float64_array, 3 * n, ab_rgb, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgb", v);
  if (want[1]) napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, ab_rgba, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgba", v);
  if (want[2]) {
    napi_create_array_with_length(env, n, &v);
    for (size_t i = 0; i < n; i++) napi_set_element(env, v, (uint32_t)i, hit_object(env, hits[i]));
    free(hits);
  } else napi_get_null(env, &v);
  napi_set_named_property(env, res, "hits", v);
  napi_value ms;
  napi_create_double(env, st.kernel_ms, &ms); napi_set_named_property(env, res, "kernel_ms", ms);
  return res;
}

// equirectTables(w, h): the panorama's tables of a w x h view (rt_view_equirect_tables)
napi_value EquirectTables(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  uint32_t w = 0, h = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_get_value_uint32(env, argv[0], &w) != napi_ok ||
      napi_get_value_uint32(env, argv[1], &h) != napi_ok || w == 0 || h == 0 || (uint64_t)w * h >= (1ull << 31)) {
    napi_throw_type_error(env, nullptr, "equirectTables(w, h): a view size with w * h below 2^31");
    return nullptr;
  }
  napi_value ab_lon, ab_lat, res, v;
  void *lon = nullptr, *lat = nullptr;
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)w * 16u, &lon, &ab_lon));
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)h * 16u, &lat, &ab_lat));
  const int rc = rt_view_equirect_tables(w, h, (double *)lon, (double *)lat);
  if (rc != RT_OK) return throw_rt(env, "rt_view_equirect_tables", rc);
  napi_create_object(env, &res);
  napi_create_typedarray(env, napi_float64_array, 2u * (size_t)w, ab_lon, 0, &v); napi_set_named_property(env, res, "lon", v);
  napi_create_typedarray(env, napi_float64_array, 2u * (size_t)h, ab_lat, 0, &v); napi_set_named_property(env, res, "lat", v);
  return res;
}

// traceView(blob, view, lon, lat, w, h, segs, wantRgb, wantRgba, wantHits): rt_trace_view.  `view` is the bytes of an rt_view whose table
// pointers are ignored: an EQUIRECT view's tables come as the two Float64Arrays.  With levels and traceRays' soft tail behind them (offs,
// nSamples, stride, base, lightRadius): rt_trace_view_soft, the soft trace of the view generated on the device; no hits.
napi_value TraceView(napi_env env, napi_callback_info info) {
  size_t argc = 16;
  napi_value argv[16];
  bool is_ta = false, is_view = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 6 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_view) != napi_ok || !is_view) {
    napi_throw_type_error(env, nullptr, "traceView(blob: Uint8Array, view: Uint8Array, lon, lat, w, h[, segs, wantRgb, wantRgba, wantHits])");
    return nullptr;
  }
  napi_typedarray_type bt, vt; napi_value ab; size_t off, blob_len = 0, view_len = 0;
  void *blob_data = nullptr, *view_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &vt, &view_len, &view_data, &ab, &off);
  uint32_t w = 0, h = 0, segs = 0;
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || vt != napi_uint8_array || view_len != sizeof(rt_view) ||
      napi_get_value_uint32(env, argv[4], &w) != napi_ok || napi_get_value_uint32(env, argv[5], &h) != napi_ok) {
    napi_throw_type_error(env, nullptr, "traceView: the blob must be a Uint8Array, the view the 136 bytes of an rt_view, w and h non-negative integers");
    return nullptr;
  }
  rt_view view;
  memcpy(&view, view_data, sizeof view);
  view.lon = view.lat = nullptr;
  size_t table_len[2] = {0, 0};
  void *table_data[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; i++) {
    bool is_table = false;
    if (napi_is_typedarray(env, argv[2 + i], &is_table) == napi_ok && is_table) {
      napi_typedarray_type tt;
      napi_get_typedarray_info(env, argv[2 + i], &tt, &table_len[i], &table_data[i], &ab, &off);
      if (tt != napi_float64_array) { table_len[i] = 0; table_data[i] = nullptr; }
    }
  }
  if (view.model == RT_VIEW_EQUIRECT && (table_len[0] != 2u * (size_t)w || table_len[1] != 2u * (size_t)h)) {
    napi_throw_type_error(env, nullptr, "traceView: an equirect view needs lon and lat, Float64Arrays of 2 w and 2 h numbers");
    return nullptr;
  }
  const bool sized = w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31);       // (anything else the library refuses: no buffer is sized from it)
  bool want[3] = {false, true, false};
  if (argc >= 7) napi_get_value_uint32(env, argv[6], &segs);
  for (size_t i = 0; i < 3 && 7 + i < argc; i++) napi_get_value_bool(env, argv[7 + i], &want[i]);
  bool soft = false;
  uint32_t levels = 0;
  struct rt_lighting la;
  const double *offs = nullptr;
  if (argc > 10) {
    napi_valuetype lt;
    napi_typeof(env, argv[10], &lt);
    soft = lt != napi_undefined && lt != napi_null;
  }
  if (soft) {
    const char *who = "traceView: soft lights are levels, offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius; no hits";
    bool unused[4];
    if (napi_get_value_uint32(env, argv[10], &levels) != napi_ok || want[2]) {
      napi_throw_type_error(env, nullptr, who);
      return nullptr;
    }
    if (!lighting_args(env, argc, argv, 11, who, &la, &offs, unused)) return nullptr;
  }
  const size_t n = sized ? (size_t)w * h : 0;
  // the library wants the blob 8-byte and the tables 16-byte aligned: one aligned copy holds all three
  const size_t blob_room = (blob_len + 15) & ~(size_t)15, lon_room = table_len[0] * 8u, lat_room = table_len[1] * 8u;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + lon_room + lat_room + 16u);
  napi_value ab_rgb = nullptr, ab_rgba = nullptr, res, v;
  void *p_rgb = nullptr, *p_rgba = nullptr;
  rt_hit *hits = (want[2] && n) ? (rt_hit *)malloc(n * sizeof(rt_hit)) : nullptr;
  if (!mem || (want[2] && n && !hits) || (want[0] && napi_create_arraybuffer(env, n * 24u, &p_rgb, &ab_rgb) != napi_ok) ||
      (want[1] && napi_create_arraybuffer(env, n * 4u, &p_rgba, &ab_rgba) != napi_ok)) {
    free(mem); free(hits);
    napi_throw_error(env, nullptr, "traceView: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  if (view.model == RT_VIEW_EQUIRECT) {
    memcpy(mem + blob_room, table_data[0], lon_room);
    memcpy(mem + blob_room + lon_room, table_data[1], lat_room);
    view.lon = (const double *)(mem + blob_room);
    view.lat = (const double *)(mem + blob_room + lon_room);
  }
  const rt_ray_outputs out = {(double *)p_rgb, (uint8_t *)p_rgba, hits};
  rt_stats st;
  const int rc = soft ? rt_trace_view_soft(mem, blob_len, &view, w, h, &la, offs, levels, segs, &out, &st) : rt_trace_view(mem, blob_len, &view, w, h, segs, &out, &st);
  free(mem);
  if (rc != RT_OK) { free(hits); return throw_rt(env, soft ? "rt_trace_view_soft" : "rt_trace_view", rc); }
  napi_create_object(env, &res);
  if (want[0]) napi_create_typedarray(env, napi_float64_array, 3 * n, ab_rgb, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgb", v);
  if (want[1]) napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, ab_rgba, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgba", v);
  if (want[2]) {
    napi_create_array_with_length(env, n, &v);
    for (size_t i = 0; i < n; i++) napi_set_element(env, v, (uint32_t)i, hit_object(env, hits[i]));
    free(hits);
  } else napi_get_null(env, &v);
  napi_set_named_property(env, res, "hits", v);
  napi_value ms;
  napi_create_double(env, st.kernel_ms, &ms); napi_set_named_property(env, res, "kernel_ms", ms);
  return res;
}

// a Float64Array argument -> its numbers (nullptr / 0 for anything else)
const double *f64_array(napi_env env, napi_value v, size_t *len) {
  bool is_ta = false;
  *len = 0;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return nullptr;
  napi_typedarray_type t; napi_value ab; size_t off; void *data = nullptr;
  napi_get_typedarray_info(env, v, &t, len, &data, &ab, &off);
  if (t != napi_float64_array) { *len = 0; return nullptr; }
  return (const double *)data;
}

// viewSamplesGrid(k): the k x k pattern (rt_view_samples_grid) as a Float64Array of 4 k k numbers: dx, dy, lu, lv per sample
napi_value ViewSamplesGrid(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  uint32_t k = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || napi_get_value_uint32(env, argv[0], &k) != napi_ok || k < 1 || k > 32) {
    napi_throw_type_error(env, nullptr, "viewSamplesGrid(k): k in 1..32");
    return nullptr;
  }
  napi_value ab, v;
  void *data = nullptr;
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)k * k * sizeof(rt_view_sample), &data, &ab));
  const int rc = rt_view_samples_grid(k, (rt_view_sample *)data);
  if (rc != RT_OK) return throw_rt(env, "rt_view_samples_grid", rc);
  NAPI_TRY(napi_create_typedarray(env, napi_float64_array, 4u * (size_t)k * k, ab, 0, &v));
  return v;
}

// equirectSampleTables(w, h, samples: Float64Array (4 per sample)) -> {lon: Float64Array (n 2 w), lat: Float64Array (n 2 h)}: one table
// per sample back to back (rt_view_equirect_sample_tables)
napi_value EquirectSampleTables(napi_env env, napi_callback_info info) {
  size_t argc = 3, len = 0;
  napi_value argv[3];
  uint32_t w = 0, h = 0;
  const double *samples = nullptr;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3 || napi_get_value_uint32(env, argv[0], &w) != napi_ok ||
      napi_get_value_uint32(env, argv[1], &h) != napi_ok || w == 0 || h == 0 || (uint64_t)w * h >= (1ull << 31) ||
      !(samples = f64_array(env, argv[2], &len)) || len == 0 || len % 4u != 0 || len / 4u > 1024u) {
    napi_throw_type_error(env, nullptr, "equirectSampleTables(w, h, samples): a view size with w * h below 2^31, a Float64Array of 4 numbers per sample, 1..1024 samples");
    return nullptr;
  }
  const uint32_t n = (uint32_t)(len / 4u);
  napi_value ab_lon, ab_lat, res, v;
  void *lon = nullptr, *lat = nullptr;
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)w * 16u * n, &lon, &ab_lon));
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)h * 16u * n, &lat, &ab_lat));
  const int rc = rt_view_equirect_sample_tables(w, h, n, (const rt_view_sample *)samples, (double *)lon, (double *)lat);
  if (rc != RT_OK) return throw_rt(env, "rt_view_equirect_sample_tables", rc);
  napi_create_object(env, &res);
  napi_create_typedarray(env, napi_float64_array, 2u * (size_t)w * n, ab_lon, 0, &v); napi_set_named_property(env, res, "lon", v);
  napi_create_typedarray(env, napi_float64_array, 2u * (size_t)h * n, ab_lat, 0, &v); napi_set_named_property(env, res, "lat", v);
  return res;
}

// traceViewSamples(blob, view, lon, lat, w, h, samples: Float64Array (4 per sample), lens: Float64Array (radius, focus) | null, segs, wantRgb,
// wantRgba): rt_trace_view_samples.  `view` as for traceView; an EQUIRECT view's tables are equirectSampleTables' for the same samples.
napi_value TraceViewSamples(napi_env env, napi_callback_info info) {
  size_t argc = 11;
  napi_value argv[11];
  bool is_ta = false, is_view = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 8 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_view) != napi_ok || !is_view) {
    napi_throw_type_error(env, nullptr, "traceViewSamples(blob: Uint8Array, view: Uint8Array, lon, lat, w, h, samples, lens[, segs, wantRgb, wantRgba])");
    return nullptr;
  }
  napi_typedarray_type bt, vt; napi_value ab; size_t off, blob_len = 0, view_len = 0;
  void *blob_data = nullptr, *view_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &vt, &view_len, &view_data, &ab, &off);
  uint32_t w = 0, h = 0, segs = 0;
  size_t table_len[2] = {0, 0}, samples_len = 0, lens_len = 0;
  const double *table_data[2] = {f64_array(env, argv[2], &table_len[0]), f64_array(env, argv[3], &table_len[1])};
  const double *samples = f64_array(env, argv[6], &samples_len), *lens_data = f64_array(env, argv[7], &lens_len);
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || vt != napi_uint8_array || view_len != sizeof(rt_view) ||
      napi_get_value_uint32(env, argv[4], &w) != napi_ok || napi_get_value_uint32(env, argv[5], &h) != napi_ok || !samples || samples_len == 0 ||
      samples_len % 4u != 0 || samples_len / 4u > 1024u || (lens_data && lens_len != 2)) {
    napi_throw_type_error(env, nullptr, "traceViewSamples: the blob must be a Uint8Array, the view the 136 bytes of an rt_view, w and h non-negative integers, "
                                        "samples a Float64Array of 4 numbers per sample (1..1024 samples), lens null or a Float64Array of 2");
    return nullptr;
  }
  const uint32_t n_samples = (uint32_t)(samples_len / 4u);
  rt_view view;
  memcpy(&view, view_data, sizeof view);
  view.lon = view.lat = nullptr;
  if (view.model == RT_VIEW_EQUIRECT && (table_len[0] != 2u * (size_t)w * n_samples || table_len[1] != 2u * (size_t)h * n_samples)) {
    napi_throw_type_error(env, nullptr, "traceViewSamples: an equirect view needs lon and lat, Float64Arrays of n 2 w and n 2 h numbers");
    return nullptr;
  }
  const bool sized = w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31);       // (anything else the library refuses: no buffer is sized from it)
  bool want[2] = {false, true};
  if (argc >= 9) napi_get_value_uint32(env, argv[8], &segs);
  for (size_t i = 0; i < 2 && 9 + i < argc; i++) napi_get_value_bool(env, argv[9 + i], &want[i]);
  const size_t n = sized ? (size_t)w * h : 0;
  // the library wants the blob 8-byte and the tables 16-byte aligned: one aligned copy holds all three
  const bool tables = view.model == RT_VIEW_EQUIRECT;
  const size_t blob_room = (blob_len + 15) & ~(size_t)15, lon_room = tables ? table_len[0] * 8u : 0, lat_room = tables ? table_len[1] * 8u : 0;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + lon_room + lat_room + 16u);
  napi_value ab_rgb = nullptr, ab_rgba = nullptr, res, v;
  void *p_rgb = nullptr, *p_rgba = nullptr;
  if (!mem || (want[0] && napi_create_arraybuffer(env, n * 24u, &p_rgb, &ab_rgb) != napi_ok) ||
      (want[1] && napi_create_arraybuffer(env, n * 4u, &p_rgba, &ab_rgba) != napi_ok)) {
    free(mem);
    napi_throw_error(env, nullptr, "traceViewSamples: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  if (tables) {
    memcpy(mem + blob_room, table_data[0], lon_room);
    memcpy(mem + blob_room + lon_room, table_data[1], lat_room);
    view.lon = (const double *)(mem + blob_room);
    view.lat = (const double *)(mem + blob_room + lon_room);
  }
  rt_view_lens lens = {0.0, 0.0};
  if (lens_data) { lens.radius = lens_data[0]; lens.focus = lens_data[1]; }
  const rt_ray_outputs out = {(double *)p_rgb, (uint8_t *)p_rgba, nullptr};
  rt_stats st;
  const int rc = rt_trace_view_samples(mem, blob_len, &view, w, h, lens_data ? &lens : nullptr, n_samples, (const rt_view_sample *)samples, segs, &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, "rt_trace_view_samples", rc);
  napi_create_object(env, &res);
  if (want[0]) napi_create_typedarray(env, napi_float64_array, 3 * n, ab_rgb, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgb", v);
  if (want[1]) napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, ab_rgba, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgba", v);
  napi_get_null(env, &v);
  napi_set_named_property(env, res, "hits", v);
  napi_value ms;
  napi_create_double(env, st.kernel_ms, &ms); napi_set_named_property(env, res, "kernel_ms", ms);
  return res;
}

// occlusion(blob, rays: Float64Array (6 per ray), length: Float64Array | null, intensity: Float64Array | null, skip: Int32Array | null,
//           wantBlocker, bin) -> {intensity: Float64Array, blocker: Int32Array | null, kernel_ms}  (rt_occlusion / rt_occlusion_binned)
napi_value Occlusion(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  bool is_ta = false, is_rays = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_rays) != napi_ok || !is_rays) {
    napi_throw_type_error(env, nullptr, "occlusion(blob: Uint8Array, rays: Float64Array[, length, intensity, skip, wantBlocker, bin])");
    return nullptr;
  }
  napi_typedarray_type bt, rt; napi_value ab; size_t off, blob_len = 0, ray_len = 0;
  void *blob_data = nullptr, *ray_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &rt, &ray_len, &ray_data, &ab, &off);
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || rt != napi_float64_array || ray_len == 0 || ray_len % 6u != 0) {
    napi_throw_type_error(env, nullptr, "occlusion: the blob must be a Uint8Array and the rays a non-empty Float64Array of 6 numbers per ray");
    return nullptr;
  }
  const size_t n = ray_len / 6u;
  // the per-ray inputs: null / undefined = the library's default, else a typed array of n elements of the right kind
  const napi_typedarray_type kinds[3] = {napi_float64_array, napi_float64_array, napi_int32_array};
  void *in_data[3] = {nullptr, nullptr, nullptr};
  for (size_t i = 0; i < 3 && 2 + i < argc; i++) {
    napi_valuetype vt;
    napi_typeof(env, argv[2 + i], &vt);
    if (vt == napi_null || vt == napi_undefined) continue;
    bool ta = false; napi_typedarray_type kt; size_t len = 0;
    if (napi_is_typedarray(env, argv[2 + i], &ta) != napi_ok || !ta || napi_get_typedarray_info(env, argv[2 + i], &kt, &len, &in_data[i], &ab, &off) != napi_ok ||
        kt != kinds[i] || len != n) {
      napi_throw_type_error(env, nullptr, "occlusion: length and intensity are Float64Arrays and skip an Int32Array of one element per ray, or null");
      return nullptr;
    }
  }
  bool want_blocker = false, bin = false;
  if (argc >= 6) napi_get_value_bool(env, argv[5], &want_blocker);
  if (argc >= 7) napi_get_value_bool(env, argv[6], &bin);
  // the library wants the blob 8-byte and the rays 16-byte aligned: one aligned copy holds both (typed arrays' own data is aligned to
  // their element size, which is what the per-ray inputs and outputs need)
  const size_t blob_room = (blob_len + 15) & ~(size_t)15;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + ((n * 48u + 15) & ~(size_t)15));
  napi_value ab_li = nullptr, ab_bl = nullptr, res, v;
  void *p_li = nullptr, *p_bl = nullptr;
  if (!mem || napi_create_arraybuffer(env, n * 8u, &p_li, &ab_li) != napi_ok || (want_blocker && napi_create_arraybuffer(env, n * 4u, &p_bl, &ab_bl) != napi_ok)) {
    free(mem);
    napi_throw_error(env, nullptr, "occlusion: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  memcpy(mem + blob_room, ray_data, n * 48u);
  const rt_occlusion_inputs in = {(const double *)in_data[0], (const double *)in_data[1], (const int32_t *)in_data[2]};
  const rt_occlusion_outputs out = {(double *)p_li, (int32_t *)p_bl};
  rt_stats st;
  const int rc = (bin ? rt_occlusion_binned : rt_occlusion)(mem, blob_len, n, (const double *)(mem + blob_room), &in, &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, bin ? "rt_occlusion_binned" : "rt_occlusion", rc);
  napi_create_object(env, &res);
  napi_create_typedarray(env, napi_float64_array, n, ab_li, 0, &v);
  napi_set_named_property(env, res, "intensity", v);
  if (want_blocker) napi_create_typedarray(env, napi_int32_array, n, ab_bl, 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "blocker", v);
  napi_value ms;
  napi_create_double(env, st.kernel_ms, &ms); napi_set_named_property(env, res, "kernel_ms", ms);
  return res;
}

// shadeRays(blob, rays: Float64Array (6 per ray), pix: Uint32Array | null, path: Uint32Array | null, bin) -> {nodes: ArrayBuffer (200 bytes
//           per ray: rt_node), count, kernel_ms}  (rt_shade_rays: one level of intersectWorld)
// relightRays(blob, rays, pix, path, bin, offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius) -> the same, the nodes' diffuse
//           and specular terms averaged over nSamples displaced copies of the lights (rt_relight_rays)
napi_value shade_or_relight(napi_env env, napi_callback_info info, bool relight) {
  size_t argc = 10;
  napi_value argv[10];
  bool is_ta = false, is_rays = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_rays) != napi_ok || !is_rays) {
    napi_throw_type_error(env, nullptr, "shadeRays(blob: Uint8Array, rays: Float64Array[, pix, path, bin])");
    return nullptr;
  }
  napi_typedarray_type bt, rt; napi_value ab; size_t off, blob_len = 0, ray_len = 0;
  void *blob_data = nullptr, *ray_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &rt, &ray_len, &ray_data, &ab, &off);
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || rt != napi_float64_array || ray_len == 0 || ray_len % 6u != 0) {
    napi_throw_type_error(env, nullptr, "shadeRays: the blob must be a Uint8Array and the rays a non-empty Float64Array of 6 numbers per ray");
    return nullptr;
  }
  const size_t n = ray_len / 6u;
  void *in_data[2] = {nullptr, nullptr};                // pix, path: null / undefined = the library's default
  for (size_t i = 0; i < 2 && 2 + i < argc; i++) {
    napi_valuetype vt;
    napi_typeof(env, argv[2 + i], &vt);
    if (vt == napi_null || vt == napi_undefined) continue;
    bool ta = false; napi_typedarray_type kt; size_t len = 0;
    if (napi_is_typedarray(env, argv[2 + i], &ta) != napi_ok || !ta || napi_get_typedarray_info(env, argv[2 + i], &kt, &len, &in_data[i], &ab, &off) != napi_ok ||
        kt != napi_uint32_array || len != n) {
      napi_throw_type_error(env, nullptr, "shadeRays: pix and path are Uint32Arrays of one element per ray, or null");
      return nullptr;
    }
  }
  bool bin = false;
  if (argc >= 5) napi_get_value_bool(env, argv[4], &bin);
  struct rt_lighting la;
  const double *offs = nullptr;
  bool unused[4];
  if (relight && !lighting_args(env, argc, argv, 5, "relightRays(blob: Uint8Array, rays: Float64Array, pix, path, bin, offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius)",
                                &la, &offs, unused))
    return nullptr;
  const size_t blob_room = (blob_len + 15) & ~(size_t)15;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + ((n * 48u + 15) & ~(size_t)15));
  napi_value ab_nodes = nullptr, res, v;
  void *p_nodes = nullptr;
  if (!mem || napi_create_arraybuffer(env, n * sizeof(rt_node), &p_nodes, &ab_nodes) != napi_ok) {
    free(mem);
    napi_throw_error(env, nullptr, "shadeRays: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  memcpy(mem + blob_room, ray_data, n * 48u);
  rt_stats st;
  const int rc = relight ? rt_relight_rays(mem, blob_len, &la, offs, n, (const double *)(mem + blob_room), (const uint32_t *)in_data[0], (const uint32_t *)in_data[1],
                                           bin ? 1 : 0, (rt_node *)p_nodes, &st)
                         : rt_shade_rays(mem, blob_len, n, (const double *)(mem + blob_room), (const uint32_t *)in_data[0], (const uint32_t *)in_data[1], bin ? 1 : 0,
                                         (rt_node *)p_nodes, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, relight ? "rt_relight_rays" : "rt_shade_rays", rc);
  napi_create_object(env, &res);
  napi_set_named_property(env, res, "nodes", ab_nodes);
  napi_create_double(env, (double)n, &v); napi_set_named_property(env, res, "count", v);
  napi_create_double(env, st.kernel_ms, &v); napi_set_named_property(env, res, "kernel_ms", v);
  return res;
}

napi_value ShadeRays(napi_env env, napi_callback_info info) { return shade_or_relight(env, info, false); }
napi_value RelightRays(napi_env env, napi_callback_info info) { return shade_or_relight(env, info, true); }

// ---- ambient occlusion (include/rt_hip.h: struct rt_ambient)
// ambientDirs(n): the cosine-weighted spiral (rt_ambient_cosine_dirs) as a Float64Array of 3 n numbers
napi_value AmbientDirs(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  uint32_t n = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || napi_get_value_uint32(env, argv[0], &n) != napi_ok || n < 1 || n > 65536) {
    napi_throw_type_error(env, nullptr, "ambientDirs(n): n in 1..65536");
    return nullptr;
  }
  napi_value ab, v;
  void *data = nullptr;
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)n * 24u, &data, &ab));
  const int rc = rt_ambient_cosine_dirs(n, (double *)data);
  if (rc != RT_OK) return throw_rt(env, "rt_ambient_cosine_dirs", rc);
  NAPI_TRY(napi_create_typedarray(env, napi_float64_array, 3u * (size_t)n, ab, 0, &v));
  return v;
}

// the tail both ambient calls share: [dirs: Float64Array (3 per entry), nSamples, stride, base, radius, wantOpen, wantIntensity, wantRgba] from
// argv[at] on -> the description, the table, the wanted outputs; false (a TypeError is pending) where an argument is of the wrong kind
bool ambient_args(napi_env env, size_t argc, napi_value *argv, size_t at, const char *who, struct rt_ambient *a, const double **dirs, bool want[3]) {
  size_t len = 0;
  double base = 0.0;
  memset(a, 0, sizeof *a);
  if (argc < at + 5 || !(*dirs = f64_array(env, argv[at], &len)) || len == 0 || len % 3u != 0 || len / 3u > 65536u ||
      napi_get_value_uint32(env, argv[at + 1], &a->n_samples) != napi_ok || napi_get_value_uint32(env, argv[at + 2], &a->stride) != napi_ok ||
      napi_get_value_double(env, argv[at + 3], &base) != napi_ok || !(base >= 0.0 && base <= 9007199254740992.0) ||
      napi_get_value_double(env, argv[at + 4], &a->radius) != napi_ok) {
    napi_throw_type_error(env, nullptr, who);
    return false;
  }
  a->n_dirs = (uint32_t)(len / 3u);
  a->base = (uint64_t)base;
  want[0] = true; want[1] = false; want[2] = false;
  for (size_t i = 0; i < 3 && at + 5 + i < argc; i++) napi_get_value_bool(env, argv[at + 5 + i], &want[i]);
  return true;
}

// {open: Float64Array | null, intensity: Float64Array | null, rgba: Uint8ClampedArray | null, kernel_ms}
napi_value ambient_result(napi_env env, size_t n, const bool want[3], napi_value ab[3], double kernel_ms) {
  napi_value res, v;
  napi_create_object(env, &res);
  if (want[0]) napi_create_typedarray(env, napi_float64_array, n, ab[0], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "open", v);
  if (want[1]) napi_create_typedarray(env, napi_float64_array, n, ab[1], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "intensity", v);
  if (want[2]) napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, ab[2], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgba", v);
  napi_create_double(env, kernel_ms, &v); napi_set_named_property(env, res, "kernel_ms", v);
  return res;
}

// ambient(blob, hits: Uint8Array (80 bytes per receiver: rt_hit), dirs, nSamples, stride, base, radius[, wantOpen, wantIntensity, wantRgba]): rt_ambient
napi_value Ambient(napi_env env, napi_callback_info info) {
  const char *who = "ambient(blob: Uint8Array, hits: Uint8Array (80 bytes per receiver), dirs: Float64Array (3 per entry), nSamples, stride, base, radius[, wantOpen, wantIntensity, wantRgba])";
  size_t argc = 10;
  napi_value argv[10];
  bool is_ta = false, is_hits = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 7 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_hits) != napi_ok || !is_hits) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  napi_typedarray_type bt, ht; napi_value ab; size_t off, blob_len = 0, hits_len = 0;
  void *blob_data = nullptr, *hits_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &ht, &hits_len, &hits_data, &ab, &off);
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || ht != napi_uint8_array || hits_len == 0 || hits_len % sizeof(rt_hit) != 0) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  struct rt_ambient a;
  const double *dirs = nullptr;
  bool want[3];
  if (!ambient_args(env, argc, argv, 2, who, &a, &dirs, want)) return nullptr;
  const size_t n = hits_len / sizeof(rt_hit);
  // the library wants the blob and the records 8-byte aligned: one aligned copy holds both
  const size_t blob_room = (blob_len + 15) & ~(size_t)15;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + ((hits_len + 15) & ~(size_t)15));
  napi_value abs[3] = {nullptr, nullptr, nullptr};
  void *p[3] = {nullptr, nullptr, nullptr};
  const size_t each[3] = {8u, 8u, 4u};
  bool ok = mem != nullptr;
  for (int i = 0; i < 3 && ok; i++) if (want[i]) ok = napi_create_arraybuffer(env, n * each[i], &p[i], &abs[i]) == napi_ok;
  if (!ok) {
    free(mem);
    napi_throw_error(env, nullptr, "ambient: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  memcpy(mem + blob_room, hits_data, hits_len);
  const rt_ambient_outputs out = {(double *)p[0], (double *)p[1], (uint32_t *)p[2]};
  rt_stats st;
  const int rc = rt_ambient(mem, blob_len, &a, dirs, n, (const rt_hit *)(mem + blob_room), &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, "rt_ambient", rc);
  return ambient_result(env, n, want, abs, st.kernel_ms);
}

// ambientView(blob, view, lon, lat, w, h, dirs, nSamples, stride, base, radius[, wantOpen, wantIntensity, wantRgba]): rt_ambient_view.  `view`,
// lon and lat as for traceView.
napi_value AmbientView(napi_env env, napi_callback_info info) {
  const char *who = "ambientView(blob: Uint8Array, view: Uint8Array, lon, lat, w, h, dirs: Float64Array (3 per entry), nSamples, stride, base, radius[, wantOpen, wantIntensity, wantRgba])";
  size_t argc = 14;
  napi_value argv[14];
  bool is_ta = false, is_view = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 11 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_view) != napi_ok || !is_view) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  napi_typedarray_type bt, vt; napi_value ab; size_t off, blob_len = 0, view_len = 0;
  void *blob_data = nullptr, *view_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &vt, &view_len, &view_data, &ab, &off);
  uint32_t w = 0, h = 0;
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || vt != napi_uint8_array || view_len != sizeof(rt_view) ||
      napi_get_value_uint32(env, argv[4], &w) != napi_ok || napi_get_value_uint32(env, argv[5], &h) != napi_ok) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  rt_view view;
  memcpy(&view, view_data, sizeof view);
  view.lon = view.lat = nullptr;
  size_t table_len[2] = {0, 0};
  const double *table_data[2] = {f64_array(env, argv[2], &table_len[0]), f64_array(env, argv[3], &table_len[1])};
  if (view.model == RT_VIEW_EQUIRECT && (table_len[0] != 2u * (size_t)w || table_len[1] != 2u * (size_t)h)) {
    napi_throw_type_error(env, nullptr, "ambientView: an equirect view needs lon and lat, Float64Arrays of 2 w and 2 h numbers");
    return nullptr;
  }
  struct rt_ambient a;
  const double *dirs = nullptr;
  bool want[3];
  if (!ambient_args(env, argc, argv, 6, who, &a, &dirs, want)) return nullptr;
  if (argc < 12) { want[0] = false; want[2] = true; }                             // (a view's default output is the picture)
  const bool sized = w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31);       // (anything else the library refuses: no buffer is sized from it)
  const size_t n = sized ? (size_t)w * h : 0;
  const size_t blob_room = (blob_len + 15) & ~(size_t)15, lon_room = table_len[0] * 8u, lat_room = table_len[1] * 8u;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + lon_room + lat_room + 16u);
  napi_value abs[3] = {nullptr, nullptr, nullptr};
  void *p[3] = {nullptr, nullptr, nullptr};
  const size_t each[3] = {8u, 8u, 4u};
  bool ok = mem != nullptr;
  for (int i = 0; i < 3 && ok; i++) if (want[i]) ok = napi_create_arraybuffer(env, n * each[i], &p[i], &abs[i]) == napi_ok;
  if (!ok) {
    free(mem);
    napi_throw_error(env, nullptr, "ambientView: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  if (view.model == RT_VIEW_EQUIRECT) {
    memcpy(mem + blob_room, table_data[0], lon_room);
    memcpy(mem + blob_room + lon_room, table_data[1], lat_room);
    view.lon = (const double *)(mem + blob_room);
    view.lat = (const double *)(mem + blob_room + lon_room);
  }
  const rt_ambient_outputs out = {(double *)p[0], (double *)p[1], (uint32_t *)p[2]};
  rt_stats st;
  const int rc = rt_ambient_view(mem, blob_len, &view, w, h, &a, dirs, &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, "rt_ambient_view", rc);
  return ambient_result(env, n, want, abs, st.kernel_ms);
}

// ---- gathered light (include/rt_hip.h: struct rt_gather)
// gather(blob, hits: Uint8Array (80 bytes per receiver), dirs, nSamples, stride, segs, base, pixBase, pixStride, wantRgb, wantRgba): rt_gather
// gatherView(blob, view, lon, lat, w, h, dirs, nSamples, stride, segs, base, pixBase, pixStride, wantRgb, wantRgba): rt_gather_view; `view`, lon
// and lat as for traceView.  -> {rgb: Float64Array (3 per receiver) | null, rgba: Uint8ClampedArray | null, kernel_ms}
napi_value gather_call(napi_env env, napi_callback_info info, bool of_view) {
  const char *who = of_view ? "gatherView(blob: Uint8Array, view: Uint8Array, lon, lat, w, h, dirs: Float64Array (3 per entry), nSamples, stride, segs, base, pixBase, pixStride, wantRgb, wantRgba)"
                            : "gather(blob: Uint8Array, hits: Uint8Array (80 bytes per receiver), dirs: Float64Array (3 per entry), nSamples, stride, segs, base, pixBase, pixStride, wantRgb, wantRgba)";
  const size_t at = of_view ? 6 : 2;                   // of dirs
  size_t argc = 15;
  napi_value argv[15];
  bool is_ta = false, is_second = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < at + 9 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_second) != napi_ok || !is_second) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  napi_typedarray_type bt, st2; napi_value ab; size_t off, blob_len = 0, second_len = 0;
  void *blob_data = nullptr, *second_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &st2, &second_len, &second_data, &ab, &off);
  uint32_t w = 0, h = 0;
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || st2 != napi_uint8_array ||
      (of_view ? second_len != sizeof(rt_view) || napi_get_value_uint32(env, argv[4], &w) != napi_ok || napi_get_value_uint32(env, argv[5], &h) != napi_ok
               : second_len == 0 || second_len % sizeof(rt_hit) != 0)) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  rt_view view;
  size_t table_len[2] = {0, 0};
  const double *table_data[2] = {nullptr, nullptr};
  if (of_view) {
    memcpy(&view, second_data, sizeof view);
    view.lon = view.lat = nullptr;
    table_data[0] = f64_array(env, argv[2], &table_len[0]); table_data[1] = f64_array(env, argv[3], &table_len[1]);
    if (view.model == RT_VIEW_EQUIRECT && (table_len[0] != 2u * (size_t)w || table_len[1] != 2u * (size_t)h)) {
      napi_throw_type_error(env, nullptr, "gatherView: an equirect view needs lon and lat, Float64Arrays of 2 w and 2 h numbers");
      return nullptr;
    }
  }
  struct rt_gather a;
  memset(&a, 0, sizeof a);
  size_t len = 0;
  double base = 0.0;
  const double *dirs = f64_array(env, argv[at], &len);
  bool want[2] = {false, false};
  if (!dirs || len == 0 || len % 3u != 0 || len / 3u > 65536u || napi_get_value_uint32(env, argv[at + 1], &a.n_samples) != napi_ok ||
      napi_get_value_uint32(env, argv[at + 2], &a.stride) != napi_ok || napi_get_value_uint32(env, argv[at + 3], &a.segs) != napi_ok ||
      napi_get_value_double(env, argv[at + 4], &base) != napi_ok || !(base >= 0.0 && base <= 9007199254740992.0) ||
      napi_get_value_uint32(env, argv[at + 5], &a.pix_base) != napi_ok || napi_get_value_uint32(env, argv[at + 6], &a.pix_stride) != napi_ok ||
      napi_get_value_bool(env, argv[at + 7], &want[0]) != napi_ok || napi_get_value_bool(env, argv[at + 8], &want[1]) != napi_ok) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  a.n_dirs = (uint32_t)(len / 3u);
  a.base = (uint64_t)base;
  const bool sized = !of_view || (w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31));   // (anything else the library refuses: no buffer is sized from it)
  const size_t n = of_view ? (sized ? (size_t)w * h : 0) : second_len / sizeof(rt_hit);
  // the library wants the blob, the records and the tables 8-byte aligned: one aligned copy holds them
  const size_t blob_room = (blob_len + 15) & ~(size_t)15, lon_room = table_len[0] * 8u, lat_room = table_len[1] * 8u;
  const size_t rest = of_view ? lon_room + lat_room + 16u : ((second_len + 15) & ~(size_t)15);
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + rest);
  napi_value abs[2] = {nullptr, nullptr};
  void *p[2] = {nullptr, nullptr};
  const size_t each[2] = {24u, 4u};
  bool ok = mem != nullptr;
  for (int i = 0; i < 2 && ok; i++) if (want[i]) ok = napi_create_arraybuffer(env, n * each[i], &p[i], &abs[i]) == napi_ok;
  if (!ok) {
    free(mem);
    napi_throw_error(env, nullptr, "gather: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  const rt_gather_outputs out = {(double *)p[0], (uint32_t *)p[1]};
  rt_stats st;
  int rc;
  if (of_view) {
    if (view.model == RT_VIEW_EQUIRECT) {
      memcpy(mem + blob_room, table_data[0], lon_room);
      memcpy(mem + blob_room + lon_room, table_data[1], lat_room);
      view.lon = (const double *)(mem + blob_room);
      view.lat = (const double *)(mem + blob_room + lon_room);
    }
    rc = rt_gather_view(mem, blob_len, &view, w, h, &a, dirs, &out, &st);
  } else {
    memcpy(mem + blob_room, second_data, second_len);
    rc = rt_gather(mem, blob_len, &a, dirs, n, (const rt_hit *)(mem + blob_room), &out, &st);
  }
  free(mem);
  if (rc != RT_OK) return throw_rt(env, of_view ? "rt_gather_view" : "rt_gather", rc);
  napi_value res, v;
  napi_create_object(env, &res);
  if (want[0]) napi_create_typedarray(env, napi_float64_array, 3 * n, abs[0], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgb", v);
  if (want[1]) napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, abs[1], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgba", v);
  napi_create_double(env, st.kernel_ms, &v); napi_set_named_property(env, res, "kernel_ms", v);
  return res;
}
napi_value Gather(napi_env env, napi_callback_info info) { return gather_call(env, info, false); }
napi_value GatherView(napi_env env, napi_callback_info info) { return gather_call(env, info, true); }

// ---- probes (include/rt_hip.h: rt_probe_outputs)
// sh9Weights(dirs: Float64Array, 3 per direction): rt_probe_sh9_weights -> Float64Array, 9 per direction
napi_value Sh9Weights(napi_env env, napi_callback_info info) {
  size_t argc = 1, len = 0;
  napi_value argv[1];
  const double *dirs = nullptr;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || !(dirs = f64_array(env, argv[0], &len)) || len == 0 || len % 3u != 0 ||
      len / 3u > 65536u) {
    napi_throw_type_error(env, nullptr, "sh9Weights(dirs: Float64Array of 3 numbers per direction, 1..65536 directions)");
    return nullptr;
  }
  napi_value ab, v;
  void *data = nullptr;
  NAPI_TRY(napi_create_arraybuffer(env, len * 24u, &data, &ab));
  const int rc = rt_probe_sh9_weights((uint32_t)(len / 3u), dirs, (double *)data);
  if (rc != RT_OK) return throw_rt(env, "rt_probe_sh9_weights", rc);
  NAPI_TRY(napi_create_typedarray(env, napi_float64_array, 3u * len, ab, 0, &v));
  return v;
}

// gatherProbes(blob, hits: Uint8Array (80 bytes per receiver), dirs, weights: Float64Array (nWeights per entry) | null, nWeights, nSamples, stride,
// segs, base, pixBase, pixStride, wantRgb, wantRgba, wantCoef): rt_gather_probes
// -> {rgb: Float64Array | null, rgba: Uint8ClampedArray | null, coef: Float64Array (3 nWeights per receiver) | null, kernel_ms}
napi_value GatherProbes(napi_env env, napi_callback_info info) {
  const char *who = "gatherProbes(blob: Uint8Array, hits: Uint8Array (80 bytes per receiver), dirs: Float64Array (3 per entry), weights: Float64Array (nWeights per entry) | null, "
                    "nWeights, nSamples, stride, segs, base, pixBase, pixStride, wantRgb, wantRgba, wantCoef)";
  size_t argc = 14;
  napi_value argv[14];
  bool is_ta = false, is_second = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 14 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_second) != napi_ok || !is_second) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  napi_typedarray_type bt, st2; napi_value ab; size_t off, blob_len = 0, hits_len = 0;
  void *blob_data = nullptr, *hits_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &st2, &hits_len, &hits_data, &ab, &off);
  struct rt_gather a;
  memset(&a, 0, sizeof a);
  size_t len = 0, wlen = 0;
  double base = 0.0;
  uint32_t n_weights = 0;
  const double *dirs = f64_array(env, argv[2], &len);
  const double *weights = f64_array(env, argv[3], &wlen);          // (null: no weights)
  bool want[3] = {false, false, false};
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || st2 != napi_uint8_array || hits_len == 0 || hits_len % sizeof(rt_hit) != 0 || !dirs || len == 0 ||
      len % 3u != 0 || len / 3u > 65536u || napi_get_value_uint32(env, argv[4], &n_weights) != napi_ok || n_weights > RT_PROBE_MAX_WEIGHTS ||
      wlen != (len / 3u) * n_weights || napi_get_value_uint32(env, argv[5], &a.n_samples) != napi_ok || napi_get_value_uint32(env, argv[6], &a.stride) != napi_ok ||
      napi_get_value_uint32(env, argv[7], &a.segs) != napi_ok || napi_get_value_double(env, argv[8], &base) != napi_ok ||
      !(base >= 0.0 && base <= 9007199254740992.0) || napi_get_value_uint32(env, argv[9], &a.pix_base) != napi_ok ||
      napi_get_value_uint32(env, argv[10], &a.pix_stride) != napi_ok || napi_get_value_bool(env, argv[11], &want[0]) != napi_ok ||
      napi_get_value_bool(env, argv[12], &want[1]) != napi_ok || napi_get_value_bool(env, argv[13], &want[2]) != napi_ok) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  a.n_dirs = (uint32_t)(len / 3u);
  a.base = (uint64_t)base;
  const size_t n = hits_len / sizeof(rt_hit);
  // the library wants the blob and the records 8-byte aligned: one aligned copy holds them
  const size_t blob_room = (blob_len + 15) & ~(size_t)15;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + ((hits_len + 15) & ~(size_t)15));
  napi_value abs[3] = {nullptr, nullptr, nullptr};
  void *p[3] = {nullptr, nullptr, nullptr};
  const size_t each[3] = {24u, 4u, 24u * (size_t)n_weights};
  bool ok = mem != nullptr;
  for (int i = 0; i < 3 && ok; i++) if (want[i]) ok = napi_create_arraybuffer(env, n * each[i], &p[i], &abs[i]) == napi_ok;
  if (!ok) {
    free(mem);
    napi_throw_error(env, nullptr, "gatherProbes: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  memcpy(mem + blob_room, hits_data, hits_len);
  const rt_probe_outputs out = {(double *)p[0], (uint32_t *)p[1], n_weights ? (double *)p[2] : nullptr};
  rt_stats st;
  const int rc = rt_gather_probes(mem, blob_len, &a, dirs, n_weights ? weights : nullptr, n_weights, n, (const rt_hit *)(mem + blob_room), &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, "rt_gather_probes", rc);
  napi_value res, v;
  napi_create_object(env, &res);
  if (want[0]) napi_create_typedarray(env, napi_float64_array, 3 * n, abs[0], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgb", v);
  if (want[1]) napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, abs[1], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "rgba", v);
  if (want[2]) napi_create_typedarray(env, napi_float64_array, 3 * n * n_weights, abs[2], 0, &v); else napi_get_null(env, &v);
  napi_set_named_property(env, res, "coef", v);
  napi_create_double(env, st.kernel_ms, &v); napi_set_named_property(env, res, "kernel_ms", v);
  return res;
}

// ---- sampled lights (include/rt_hip.h: struct rt_lighting)
// lightingOffsets(n): the spiral over the unit sphere (rt_lighting_sphere_offsets) as a Float64Array of 3 n numbers
napi_value LightingOffsets(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  uint32_t n = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || napi_get_value_uint32(env, argv[0], &n) != napi_ok || n < 1 || n > 65536) {
    napi_throw_type_error(env, nullptr, "lightingOffsets(n): n in 1..65536");
    return nullptr;
  }
  napi_value ab, v;
  void *data = nullptr;
  NAPI_TRY(napi_create_arraybuffer(env, (size_t)n * 24u, &data, &ab));
  const int rc = rt_lighting_sphere_offsets(n, (double *)data);
  if (rc != RT_OK) return throw_rt(env, "rt_lighting_sphere_offsets", rc);
  NAPI_TRY(napi_create_typedarray(env, napi_float64_array, 3u * (size_t)n, ab, 0, &v));
  return v;
}

// the tail both lighting calls share: [offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius, wantDiffuse, wantIntensity, wantLit,
// wantRgba] from argv[at] on -> the description, the table, the wanted outputs; false (a TypeError is pending) where an argument is of the wrong kind
bool lighting_args(napi_env env, size_t argc, napi_value *argv, size_t at, const char *who, struct rt_lighting *a, const double **offs, bool want[4]) {
  size_t len = 0;
  double base = 0.0;
  memset(a, 0, sizeof *a);
  if (argc < at + 5 || !(*offs = f64_array(env, argv[at], &len)) || len == 0 || len % 3u != 0 || len / 3u > 65536u ||
      napi_get_value_uint32(env, argv[at + 1], &a->n_samples) != napi_ok || napi_get_value_uint32(env, argv[at + 2], &a->stride) != napi_ok ||
      napi_get_value_double(env, argv[at + 3], &base) != napi_ok || !(base >= 0.0 && base <= 9007199254740992.0) ||
      napi_get_value_double(env, argv[at + 4], &a->light_radius) != napi_ok) {
    napi_throw_type_error(env, nullptr, who);
    return false;
  }
  a->n_offs = (uint32_t)(len / 3u);
  a->base = (uint64_t)base;
  want[0] = true; want[1] = false; want[2] = false; want[3] = false;
  for (size_t i = 0; i < 4 && at + 5 + i < argc; i++) napi_get_value_bool(env, argv[at + 5 + i], &want[i]);
  return true;
}

// {diffuse, intensity, lit: Float64Array | null, rgba: Uint8ClampedArray | null, kernel_ms}
napi_value lighting_result(napi_env env, size_t n, const bool want[4], napi_value ab[4], double kernel_ms) {
  static const char *const names[4] = {"diffuse", "intensity", "lit", "rgba"};
  napi_value res, v;
  napi_create_object(env, &res);
  for (int i = 0; i < 4; i++) {
    if (!want[i]) napi_get_null(env, &v);
    else if (i < 3) napi_create_typedarray(env, napi_float64_array, n, ab[i], 0, &v);
    else napi_create_typedarray(env, napi_uint8_clamped_array, 4 * n, ab[i], 0, &v);
    napi_set_named_property(env, res, names[i], v);
  }
  napi_create_double(env, kernel_ms, &v); napi_set_named_property(env, res, "kernel_ms", v);
  return res;
}

// lighting(blob, hits: Uint8Array (80 bytes per receiver: rt_hit), offs, nSamples, stride, base, lightRadius[, wantDiffuse, wantIntensity, wantLit, wantRgba]): rt_lighting
napi_value Lighting(napi_env env, napi_callback_info info) {
  const char *who = "lighting(blob: Uint8Array, hits: Uint8Array (80 bytes per receiver), offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius[, wantDiffuse, wantIntensity, wantLit, wantRgba])";
  size_t argc = 11;
  napi_value argv[11];
  bool is_ta = false, is_hits = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 7 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_hits) != napi_ok || !is_hits) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  napi_typedarray_type bt, ht; napi_value ab; size_t off, blob_len = 0, hits_len = 0;
  void *blob_data = nullptr, *hits_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &ht, &hits_len, &hits_data, &ab, &off);
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || ht != napi_uint8_array || hits_len == 0 || hits_len % sizeof(rt_hit) != 0) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  struct rt_lighting a;
  const double *offs = nullptr;
  bool want[4];
  if (!lighting_args(env, argc, argv, 2, who, &a, &offs, want)) return nullptr;
  const size_t n = hits_len / sizeof(rt_hit);
  // the library wants the blob and the records 8-byte aligned: one aligned copy holds both
  const size_t blob_room = (blob_len + 15) & ~(size_t)15;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + ((hits_len + 15) & ~(size_t)15));
  napi_value abs[4] = {nullptr, nullptr, nullptr, nullptr};
  void *p[4] = {nullptr, nullptr, nullptr, nullptr};
  const size_t each[4] = {8u, 8u, 8u, 4u};
  bool ok = mem != nullptr;
  for (int i = 0; i < 4 && ok; i++) if (want[i]) ok = napi_create_arraybuffer(env, n * each[i], &p[i], &abs[i]) == napi_ok;
  if (!ok) {
    free(mem);
    napi_throw_error(env, nullptr, "lighting: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  memcpy(mem + blob_room, hits_data, hits_len);
  const rt_lighting_outputs out = {(double *)p[0], (double *)p[1], (double *)p[2], (uint32_t *)p[3]};
  rt_stats st;
  const int rc = rt_lighting(mem, blob_len, &a, offs, n, (const rt_hit *)(mem + blob_room), &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, "rt_lighting", rc);
  return lighting_result(env, n, want, abs, st.kernel_ms);
}

// lightingView(blob, view, lon, lat, w, h, offs, nSamples, stride, base, lightRadius[, wantDiffuse, wantIntensity, wantLit, wantRgba]): rt_lighting_view.
// `view`, lon and lat as for traceView.
napi_value LightingView(napi_env env, napi_callback_info info) {
  const char *who = "lightingView(blob: Uint8Array, view: Uint8Array, lon, lat, w, h, offs: Float64Array (3 per entry), nSamples, stride, base, lightRadius[, wantDiffuse, wantIntensity, wantLit, wantRgba])";
  size_t argc = 15;
  napi_value argv[15];
  bool is_ta = false, is_view = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 11 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
      napi_is_typedarray(env, argv[1], &is_view) != napi_ok || !is_view) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  napi_typedarray_type bt, vt; napi_value ab; size_t off, blob_len = 0, view_len = 0;
  void *blob_data = nullptr, *view_data = nullptr;
  napi_get_typedarray_info(env, argv[0], &bt, &blob_len, &blob_data, &ab, &off);
  napi_get_typedarray_info(env, argv[1], &vt, &view_len, &view_data, &ab, &off);
  uint32_t w = 0, h = 0;
  if ((bt != napi_uint8_array && bt != napi_uint8_clamped_array) || vt != napi_uint8_array || view_len != sizeof(rt_view) ||
      napi_get_value_uint32(env, argv[4], &w) != napi_ok || napi_get_value_uint32(env, argv[5], &h) != napi_ok) {
    napi_throw_type_error(env, nullptr, who);
    return nullptr;
  }
  rt_view view;
  memcpy(&view, view_data, sizeof view);
  view.lon = view.lat = nullptr;
  size_t table_len[2] = {0, 0};
  const double *table_data[2] = {f64_array(env, argv[2], &table_len[0]), f64_array(env, argv[3], &table_len[1])};
  if (view.model == RT_VIEW_EQUIRECT && (table_len[0] != 2u * (size_t)w || table_len[1] != 2u * (size_t)h)) {
    napi_throw_type_error(env, nullptr, "lightingView: an equirect view needs lon and lat, Float64Arrays of 2 w and 2 h numbers");
    return nullptr;
  }
  struct rt_lighting a;
  const double *offs = nullptr;
  bool want[4];
  if (!lighting_args(env, argc, argv, 6, who, &a, &offs, want)) return nullptr;
  if (argc < 12) { want[0] = false; want[3] = true; }                             // (a view's default output is the picture)
  const bool sized = w != 0 && h != 0 && (uint64_t)w * h < (1ull << 31);       // (anything else the library refuses: no buffer is sized from it)
  const size_t n = sized ? (size_t)w * h : 0;
  const size_t blob_room = (blob_len + 15) & ~(size_t)15, lon_room = table_len[0] * 8u, lat_room = table_len[1] * 8u;
  uint8_t *mem = (uint8_t *)aligned_alloc(16, blob_room + lon_room + lat_room + 16u);
  napi_value abs[4] = {nullptr, nullptr, nullptr, nullptr};
  void *p[4] = {nullptr, nullptr, nullptr, nullptr};
  const size_t each[4] = {8u, 8u, 8u, 4u};
  bool ok = mem != nullptr;
  for (int i = 0; i < 4 && ok; i++) if (want[i]) ok = napi_create_arraybuffer(env, n * each[i], &p[i], &abs[i]) == napi_ok;
  if (!ok) {
    free(mem);
    napi_throw_error(env, nullptr, "lightingView: out of memory");
    return nullptr;
  }
  memcpy(mem, blob_data, blob_len);
  if (view.model == RT_VIEW_EQUIRECT) {
    memcpy(mem + blob_room, table_data[0], lon_room);
    memcpy(mem + blob_room + lon_room, table_data[1], lat_room);
    view.lon = (const double *)(mem + blob_room);
    view.lat = (const double *)(mem + blob_room + lon_room);
  }
  const rt_lighting_outputs out = {(double *)p[0], (double *)p[1], (double *)p[2], (uint32_t *)p[3]};
  rt_stats st;
  const int rc = rt_lighting_view(mem, blob_len, &view, w, h, &a, offs, &out, &st);
  free(mem);
  if (rc != RT_OK) return throw_rt(env, "rt_lighting_view", rc);
  return lighting_result(env, n, want, abs, st.kernel_ms);
}

napi_value Module(napi_env env, napi_value exports) {
  const napi_property_descriptor props[] = {
      {"init", nullptr, Init, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"render", nullptr, Render, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"renderAsync", nullptr, RenderAsync, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"renderAdaptive", nullptr, RenderAdaptive, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"renderProgressive", nullptr, RenderProgressive, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"validate", nullptr, Validate, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"shutdown", nullptr, Shutdown, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"abiVersion", nullptr, AbiVersion, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"buildId", nullptr, BuildId, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"renderHits", nullptr, RenderHits, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"pick", nullptr, Pick, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"traceRays", nullptr, TraceRays, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"occlusion", nullptr, Occlusion, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"shadeRays", nullptr, ShadeRays, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"relightRays", nullptr, RelightRays, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"traceView", nullptr, TraceView, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"equirectTables", nullptr, EquirectTables, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"viewSamplesGrid", nullptr, ViewSamplesGrid, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"equirectSampleTables", nullptr, EquirectSampleTables, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"traceViewSamples", nullptr, TraceViewSamples, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ambientDirs", nullptr, AmbientDirs, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ambient", nullptr, Ambient, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ambientView", nullptr, AmbientView, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"gather", nullptr, Gather, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"gatherView", nullptr, GatherView, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"gatherProbes", nullptr, GatherProbes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"sh9Weights", nullptr, Sh9Weights, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"lightingOffsets", nullptr, LightingOffsets, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"lighting", nullptr, Lighting, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"lightingView", nullptr, LightingView, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
  return exports;
}

}  // namespace

NAPI_MODULE(rt_napi, Module)
