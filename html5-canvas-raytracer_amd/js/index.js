'use strict';
// render(width, height, scene) — the drop-in entry point for the reference's per-pixel path
// (redraw()/spanish() + intersectWorld, /root/reference/main.js:180-201, :216-451), backed by the
// MI355X HIP kernel through the N-API shim.  The returned Uint8ClampedArray has the layout of
// ImageData.data (main.js:83, :195-198), so it drops in behind the canvas:
//     ctx.putImageData(new ImageData(render(w, h, scene), w, h), 0, 0)
// There is NO JavaScript rendering fallback here: if the addon or the GPU is missing, this throws.

const path = require('path');
const {flattenScene} = require('./flatten.js');
const scene = require('./scene.js');
const scenes = require('./scenes.js');

let addon = null;
function native() {
  if (addon) return addon;
  const p = path.join(__dirname, '..', 'napi', 'rt_napi.node');
  try { addon = require(p); } catch (e) {
    throw new Error('html5-canvas-raytracer_amd: native addon ' + p + ' is not built or cannot load (' + e.message +
      '); run `python -c "import __graft_entry__ as g; g.build()"`. There is no CPU fallback for render().');
  }
  return addon;
}

const FLAG_COUNT = 1, FLAG_STRICT_FP = 2;
let inited = false;
// maxDevices: GPUs rt_render may shard one frame over (RCCL gather); default 1.  Pass 0 for every visible GPU.
function init(maxDevices) { const n = native().init(maxDevices === undefined ? 1 : maxDevices); inited = true; return n; }
function flagsOf(opts) { return ((opts && opts.count) ? FLAG_COUNT : 0) | ((opts && opts.strictFp) ? FLAG_STRICT_FP : 0); }

// -> Uint8ClampedArray of length 4*width*height over a pinned host buffer; `.stats` carries timings.
// opts.into: the frame to fill instead of a new one - the reference creates its ImageData once (main.js:83) and every redraw
// writes into it again (main.js:195-200).  Hand in what an earlier render() returned (pinned memory: the GPU stores into it
// directly, nothing is allocated) - or any Uint8ClampedArray of 4*width*height bytes, e.g. a canvas ImageData.data (pageable
// memory: the frame is copied out of the GPU's memory, about half the rate).  Returns that same array.
// opts.adaptive: {k, threshold} - adaptive supersampling: the frame of a scene whose own supersample is 1, with k x k samples (k 2..4,
// default 4) for the pixels that differ from a 4-neighbour by `threshold` (0..256, default 32) or more in R, G or B; `.stats.refined`
// says how many pixels that were.  On one GPU.
function adaptiveOf(opts) {
  const a = opts && opts.adaptive;
  if (!a) return null;
  return {k: a.k === undefined ? 4 : a.k, threshold: a.threshold === undefined ? 32 : a.threshold};
}
function render(width, height, sceneObj, opts) {
  if (!inited) init(opts && opts.maxDevices);
  const ad = adaptiveOf(opts);
  const r = ad ? native().renderAdaptive(flattenScene(sceneObj), width, height, flagsOf(opts), ad.k, ad.threshold, (opts && opts.into) || undefined)
    : native().render(flattenScene(sceneObj), width, height, flagsOf(opts), (opts && opts.into) || undefined);
  r.data.stats = r.stats;
  return r.data;
}

// Promise variant: the launch and the copy-out run off the event loop (napi_async_work)
function renderAsync(width, height, sceneObj, opts) {
  try { if (!inited) init(opts && opts.maxDevices); } catch (e) { return Promise.reject(e); }
  const ad = adaptiveOf(opts);
  const p = ad ? native().renderAdaptive(flattenScene(sceneObj), width, height, flagsOf(opts), ad.k, ad.threshold, undefined, true)
    : native().renderAsync(flattenScene(sceneObj), width, height, flagsOf(opts));
  return p.then((r) => { r.data.stats = r.stats; return r.data; });
}

// Progressive variant: the reference shows its frame row by row (one spanish(y) per macrotask, main.js:183-201); here
// the frame is rendered as `bands` row bands (default 8, at most 64) and onBand({firstRow, rows, data}) fires on the main
// thread as each band lands in the frame buffer - `data` is the view of just those rows, `frame` the whole buffer that
// is being filled (usable with putImageData(..., dirtyY) while it fills).  Resolves to the full frame.
function renderProgressive(width, height, sceneObj, opts) {
  try { if (!inited) init(opts && opts.maxDevices); } catch (e) { return Promise.reject(e); }
  const bands = (opts && opts.bands) || 8;
  const onBand = (opts && opts.onBand) || (() => {});
  let r;
  try {
    r = native().renderProgressive(flattenScene(sceneObj), width, height, flagsOf(opts), bands,
      (firstRow, rows) => onBand({firstRow, rows, frame: r.data, data: r.data.subarray(firstRow * width * 4, (firstRow + rows) * width * 4)}));
  } catch (e) { return Promise.reject(e); }
  return r.promise.then((stats) => { r.data.stats = stats; return r.data; });
}

// What is under the samples (main.js:216-231, 440-449, which the reference computes per ray and drops after shading): the primary
// hit of every sample of the frame's sample grid (k*width x k*height when the scene supersamples by k), row-major:
//   id      Int32Array, the index into scene.objects | inside << 16, or -1 where the ray meets nothing (main.js:231)
//   depth   Float64Array, hit.t (Infinity on a miss)                  opts.depth === false: not computed (null)
//   normal  Float32Array, 3 per sample, hit.n (0,0,0 on a miss)        opts.normal === false: not computed (null)
function renderHits(width, height, sceneObj, opts) {
  if (!inited) init(opts && opts.maxDevices);
  return native().renderHits(flattenScene(sceneObj), width, height, !(opts && opts.depth === false), !(opts && opts.normal === false));
}

// Pixel picking: what is under output pixel (x, y) - clicking on the canvas.  The pixel's sample is the centre one of its k x k block,
// (k*x + floor(k/2), k*y + floor(k/2)).  Returns {index, object: scene.objects[index], inside, t, point, normal, u, v} (hit.u / hit.v
// of main.js:446-447), or null when the ray meets nothing.  Throws for a pixel outside the frame.
function pick(width, height, sceneObj, x, y) {
  if (!(Number.isInteger(x) && Number.isInteger(y) && x >= 0 && y >= 0 && x < width && y < height)) {
    throw new RangeError('pick: (' + x + ', ' + y + ') is not a pixel of the ' + width + 'x' + height + ' frame');
  }
  if (!inited) init();
  const k = sceneObj.supersample || 1, c = Math.floor(k / 2);
  const r = native().pick(flattenScene(sceneObj), width, height, k * x + c, k * y + c);
  if (r) r.object = sceneObj.objects[r.index];
  return r;
}

// The reference's normal3D (main.js:62-66): v * (1 / |v|); the zero vector is returned unchanged.
function normal3D(v) {
  const l = Math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (l === 0) return [v[0], v[1], v[2]];
  const k = 1 / l;
  return [v[0] * k, v[1] * k, v[2] * k];
}

// The primary rays of the width x height frame, main.js:184-193 operation for operation, as a Float64Array of 6 numbers per sample
// {org, dir} in row order of the k*width x k*height sample grid: traceRays of this list is the scene's strict-arithmetic sample
// frame, stars included (a ray's index in the list is its sample's index in the frame).
function primaryRays(width, height, sceneObj) {
  const k = sceneObj.supersample || 1, sw = k * width, sh = k * height;
  const {origin, axisX, axisY, axisZ} = sceneObj.camera;
  const fov = sceneObj.fovDeg === undefined ? 60 : sceneObj.fovDeg;
  const projA = fov * Math.PI / 180, projW = sw / 2, projH = sh / 2, projD = projW / tanHalf(projA);
  const rays = new Float64Array(6 * sw * sh);
  let i = 0;
  for (let y = 0; y < sh; y++) {
    for (let x = 0; x < sw; x++) {
      const dist = [x - projW + 0.5, projH - y - 0.5, projD];
      const target = [
        origin[0] + axisX[0] * dist[0] + axisY[0] * dist[0] + axisZ[0] * dist[0],
        origin[1] + axisX[1] * dist[1] + axisY[1] * dist[1] + axisZ[1] * dist[1],
        origin[2] + axisX[2] * dist[2] + axisY[2] * dist[2] + axisZ[2] * dist[2]];
      const ray = normal3D([target[0] - origin[0], target[1] - origin[1], target[2] - origin[2]]);
      rays[i++] = origin[0]; rays[i++] = origin[1]; rays[i++] = origin[2];
      rays[i++] = ray[0]; rays[i++] = ray[1]; rays[i++] = ray[2];
    }
  }
  return rays;
}
function tanHalf(projA) { return Math.tan(projA / 2); }

// intersectWorld(segs, objects, org, dir) (main.js:216-336) for a list of rays: `rays` is a Float64Array of 6 numbers per ray
// {org, dir}, directions used as given (normal3D above is the reference's).  opts: segs (0 / undefined = the scene's depth) and which
// outputs to compute - rgb (default true) Float64Array 3 per ray, rgba Uint8ClampedArray 4 per ray, hits Array of pick's records
// (null = a miss).  The scene's camera plays no part.  A ray with a non-finite component is not traced: NaN x 3 / 0, 0, 0, 255 / null.
// opts.bin: the GPU puts each chunk of 2^18 rays into an order in which neighbours in a wave are neighbours in space before it traces
// them (rt_trace_rays_binned) - the same results, sooner for a list that is not coherent (scattered probes, collected secondary rays).
// opts.wavefront: level by level through shade, spawn and fold (rt_trace_rays_wavefront) instead of the one recursive kernel - the same
// bytes in rgb and rgba, no hits, plus levelCounts (the rays shaded per level); opts.orderLevels bins every level after the first.
// opts.soft: {samples, lightRadius, offsets, stride, levels, base} - the wavefront form with lights that have a size (rt_trace_rays_soft):
// the diffuse and specular terms of the nodes of the first `levels` levels (default 1: what the rays hit; the scene's depth: every
// bounce) are means over `samples` runs of the light loop, every light displaced by lightRadius times an entry of offsets (default
// lightingOffsets(samples) with stride 0: every ray the same entries; with offsets, stride defaults to 1 and ray i walks the table from
// (base + i) * stride; relightRays' stride defaults to 1 either way).  No hits, no bin.
// opts.soft.method: 'wavefront' (the default) or 'recursive' - the same picture from one launch per chunk of 2^18 rays, a per-lane stack
// in place of the nodes in device memory (rt_trace_rays_soft_recursive): the same bytes, no levelCounts, and {bin: true} is allowed.
function softOf(o, who, walks) {
  const s = o.soft;
  if (s === null || typeof s !== 'object' || !Number.isInteger(s.samples) || s.samples < 1 || typeof s.lightRadius !== 'number' ||
      (s.offsets != null && !(s.offsets instanceof Float64Array && s.offsets.length > 0 && s.offsets.length % 3 === 0)) ||
      (s.stride != null && !(Number.isInteger(s.stride) && s.stride >= 0)) || (s.levels != null && !(Number.isInteger(s.levels) && s.levels >= 0)) ||
      (s.base != null && !(Number.isInteger(s.base) && s.base >= 0)) || (s.method != null && s.method !== 'wavefront' && s.method !== 'recursive')) {
    throw new TypeError(who + ": soft is {samples: integer >= 1, lightRadius: number[, offsets: Float64Array of 3 numbers per entry, stride, levels, base, method: 'wavefront' | 'recursive']}");
  }
  const offs = s.offsets || native().lightingOffsets(s.samples);
  return {recursive: s.method === 'recursive', levels: s.levels == null ? 1 : s.levels, tail: [offs, s.samples, s.stride != null ? s.stride : (s.offsets || walks ? 1 : 0), s.base || 0, s.lightRadius]};
}
function traceRays(sceneObj, rays, opts) {
  if (!(rays instanceof Float64Array) || rays.length === 0 || rays.length % 6 !== 0) {
    throw new TypeError('traceRays: rays must be a non-empty Float64Array of 6 numbers per ray');
  }
  if (!inited) init(opts && opts.maxDevices);
  const o = opts || {};
  if (o.wavefront && (o.hits || o.bin)) throw new TypeError('traceRays: {wavefront: true} returns no hits and takes no {bin: true} (orderLevels bins the later levels)');
  const soft = o.soft !== undefined ? softOf(o, 'traceRays') : null;
  if (soft && (o.hits || (o.bin && !soft.recursive))) throw new TypeError("traceRays: {soft} returns no hits and takes {bin: true} with method 'recursive' only");
  if (soft && soft.recursive && (o.wavefront || o.orderLevels)) throw new TypeError("traceRays: {soft: {method: 'recursive'}} is not the wavefront form");
  const args = [new Uint8Array(flattenScene(sceneObj)), rays, o.segs || 0, o.rgb !== false, !!o.rgba, !!o.hits, !!o.bin, !!o.wavefront, !!o.orderLevels];
  const r = soft ? native().traceRays(...args, soft.levels, ...soft.tail, soft.recursive) : native().traceRays(...args);
  if (r.hits) for (const h of r.hits) if (h) h.object = sceneObj.objects[h.index];
  return r;
}

// Views: a camera's rays generated on the GPU (include/rt_hip.h: rt_view).  traceRays renders any projection, but its list is built
// here and crosses the link at 48 bytes per ray; a view is the list's description - a model, an origin, a basis - and the library
// generates the rays on the device in front of the same trace.  The constructors take the axes as given: image x runs along axisX,
// image y (upwards) along axisY, the view looks along axisZ (lookAt's axisX, main.js:95, points to the viewer's LEFT).
//   views.reference(origin, axisX, axisY, axisZ, fovDeg)  the reference's own per-component rays (main.js:186-193): the strict frame's
//   views.pinhole(origin, axisX, axisY, axisZ, fovDeg)    a true pinhole for any basis
//   views.ortho(origin, axisX, axisY, axisZ, scale)       parallel rays along axisZ, `scale` world units per pixel
//   views.equirect(origin, axisX, axisY, axisZ, w, h)     a w x h panorama; its tables (sines and cosines per column and per row) are
//                                                         filled through the addon, for that size
//   views.cubeFaces(eye)         six pinholes of 90 degrees for square frames, +x -x +y -y +z -z; axisX = axisZ x axisY, up = +y for the
//                                side faces, +z for +y and -z for -y (rt_host.cube_views states each basis)
//   views.stereo(view, separation)   [left, right]: origins moved by -/+ separation / 2 along unit(axisX)
//   views.bytes(view)            the 136 bytes of the rt_view record (table pointers zero): what Python's rt_host.view(...) holds
const VIEW_REFERENCE = 0, VIEW_PINHOLE = 1, VIEW_ORTHO = 2, VIEW_EQUIRECT = 3, VIEW_BYTES = 136;
function makeView(model, origin, axisX, axisY, axisZ, fovDeg, scale) {
  const v3 = (a) => [Number(a[0]), Number(a[1]), Number(a[2])];
  return {model, origin: v3(origin), axisX: v3(axisX), axisY: v3(axisY), axisZ: v3(axisZ), fovDeg: fovDeg === undefined ? 60 : fovDeg,
    scale: scale === undefined ? 1 : scale, lon: null, lat: null};
}
function viewBytes(view) {
  const buf = new Uint8Array(VIEW_BYTES), d = new DataView(buf.buffer);
  d.setUint32(0, view.model, true);
  [view.origin, view.axisX, view.axisY, view.axisZ].forEach((a, i) => { for (let c = 0; c < 3; c++) d.setFloat64(8 + 24 * i + 8 * c, a[c], true); });
  d.setFloat64(104, view.fovDeg, true);
  d.setFloat64(112, view.scale, true);
  return buf;
}
const views = {
  REFERENCE: VIEW_REFERENCE, PINHOLE: VIEW_PINHOLE, ORTHO: VIEW_ORTHO, EQUIRECT: VIEW_EQUIRECT,
  reference: (origin, axisX, axisY, axisZ, fovDeg) => makeView(VIEW_REFERENCE, origin, axisX, axisY, axisZ, fovDeg),
  pinhole: (origin, axisX, axisY, axisZ, fovDeg) => makeView(VIEW_PINHOLE, origin, axisX, axisY, axisZ, fovDeg),
  ortho: (origin, axisX, axisY, axisZ, scale) => makeView(VIEW_ORTHO, origin, axisX, axisY, axisZ, undefined, scale),
  equirect: (origin, axisX, axisY, axisZ, w, h) => Object.assign(makeView(VIEW_EQUIRECT, origin, axisX, axisY, axisZ), native().equirectTables(w, h)),
  cubeFaces: (eye) => [[[0, 0, 1], [0, 1, 0], [1, 0, 0]], [[0, 0, -1], [0, 1, 0], [-1, 0, 0]], [[1, 0, 0], [0, 0, 1], [0, 1, 0]],
    [[1, 0, 0], [0, 0, -1], [0, -1, 0]], [[-1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0], [0, 0, -1]]]
    .map(([ax, ay, az]) => makeView(VIEW_PINHOLE, eye, ax, ay, az, 90)),
  stereo: (view, separation) => {
    const u = normal3D(view.axisX), half = separation / 2;
    return [-1, 1].map((s) => Object.assign({}, view, {origin: view.origin.map((o, c) => (s < 0 ? o - u[c] * half : o + u[c] * half))}));
  },
  bytes: viewBytes,
  // sampled views (include/rt_hip.h: rt_view_sample, rt_view_lens)
  //   views.sampleGrid(k)         the k x k pattern, k in 1..32, through the library (rt_view_samples_grid): [{dx, dy, lu, lv}], sub-pixel
  //                               offsets in pixels (dy downwards) and their concentric map onto the unit disk - one pattern for
  //                               antialiasing and the lens
  //   views.lens(radius, focus)   a thin lens for a pinhole view, focused on the plane `focus` away along axisZ
  sampleGrid: (k) => {
    const a = native().viewSamplesGrid(k);
    return Array.from({length: a.length / 4}, (_, i) => ({dx: a[4 * i], dy: a[4 * i + 1], lu: a[4 * i + 2], lv: a[4 * i + 3]}));
  },
  lens: (radius, focus) => ({radius: Number(radius), focus: Number(focus)}),
};

function packSamples(samples) {
  if (samples instanceof Float64Array) return samples;
  const a = new Float64Array(4 * samples.length);
  samples.forEach((s, i) => { a[4 * i] = s.dx || 0; a[4 * i + 1] = s.dy || 0; a[4 * i + 2] = s.lu || 0; a[4 * i + 3] = s.lv || 0; });
  return a;
}

// intersectWorld for every ray of `view` at w x h, in frame order (ray y w + x): traceRays' result shape.  opts: segs, and which
// outputs to compute - rgba (default true) the Uint8ClampedArray that is a w x h ImageData.data, rgb Float64Array 3 per ray, hits.
// The scene's own camera plays no part.
// opts.samples (views.sampleGrid(k), or the caller's own [{dx, dy, lu, lv}]) and / or opts.lens (views.lens, pinhole views): one trace
// per sample, averaged on the GPU in binary64 (rt_trace_view_samples) - rgb is the mean, rgba the mean through the store rule; no hits.
// A lens without samples takes the one zero sample: the pinhole itself.
// opts.soft: {samples, lightRadius, offsets, stride, levels} as traceRays takes them - the soft trace of the view, its rays generated on
// the device and each chunk of rows one launch (rt_trace_view_soft); no hits, no samples or lens.
function traceView(sceneObj, view, w, h, opts) {
  if (!view || !Number.isInteger(view.model)) throw new TypeError('traceView: view must come from views.reference / pinhole / ortho / equirect');
  if (!inited) init(opts && opts.maxDevices);
  const o = opts || {};
  if (o.soft !== undefined && (o.hits || o.samples || o.lens)) throw new TypeError('traceView: {soft} returns no hits and takes no samples or lens');
  if (o.samples || o.lens) {
    if (o.hits) throw new TypeError('traceView: a sampled view returns no hits (a mean of hit records means nothing)');
    const samples = packSamples(o.samples || [{dx: 0, dy: 0, lu: 0, lv: 0}]);
    const t = view.model === VIEW_EQUIRECT ? native().equirectSampleTables(w, h, samples) : {lon: null, lat: null};
    return native().traceViewSamples(new Uint8Array(flattenScene(sceneObj)), viewBytes(view), t.lon, t.lat, w, h, samples,
      o.lens ? new Float64Array([o.lens.radius, o.lens.focus]) : null, o.segs || 0, !!o.rgb, o.rgba !== false);
  }
  const soft = o.soft !== undefined ? softOf({soft: Object.assign({}, o.soft, {base: 0, method: undefined})}, 'traceView') : null;
  const r = native().traceView(new Uint8Array(flattenScene(sceneObj)), viewBytes(view), view.lon || null, view.lat || null, w, h, o.segs || 0,
    !!o.rgb, o.rgba !== false, !!o.hits, ...(soft ? [soft.levels, ...soft.tail] : []));
  if (r.hits) for (const hit of r.hits) if (hit) hit.object = sceneObj.objects[hit.index];
  return r;
}

// One level of intersectWorld (main.js:216-336 WITHOUT its two recursive calls) for a list of rays: {nodes: ArrayBuffer of 200-byte
// rt_node records (include/rt_hip.h), count, node(i)}.  opts: pix, path (Uint32Array per ray: the stars sampler's; default i and 1),
// bin (the GPU orders the list first - the same nodes).  node(i) reads record i: {hit: pick's record or null, sample, diffuse,
// specular, ambient, reflectWeight, refractWeight, reflectDir, refractDir, children (bit 0 reflect, bit 1 refract)}; the child rays
// start at hit.point.
const NODE_BYTES = 200;
function nodeAt(buf, i, sceneObj) {
  const d = new DataView(buf, i * NODE_BYTES, NODE_BYTES);
  const f = (off) => d.getFloat64(off, true), v3 = (off) => [f(off), f(off + 8), f(off + 16)];
  const index = d.getInt32(0, true);
  const hit = index < 0 ? null : {index, inside: d.getInt32(4, true) !== 0, t: f(8), point: v3(16), normal: v3(40), u: f(64), v: f(72), object: sceneObj.objects[index]};
  return {hit, sample: v3(80), diffuse: f(104), specular: f(112), ambient: f(120), reflectWeight: f(128), refractWeight: f(136),
    reflectDir: v3(144), refractDir: v3(168), children: d.getUint32(192, true)};
}
// relightRays(scene, rays, opts): shadeRays' result with soft lights (rt_relight_rays) - opts as shadeRays takes them, and samples,
// lightRadius, offsets, stride, base as traceRays' opts.soft names them; sample s of ray i uses entry ((base + pix_i) stride + s) % n_offs.
function shadeRays(sceneObj, rays, opts) { return shadeOrRelight('shadeRays', sceneObj, rays, opts, false); }
function relightRays(sceneObj, rays, opts) { return shadeOrRelight('relightRays', sceneObj, rays, opts, true); }
function shadeOrRelight(who, sceneObj, rays, opts, relight) {
  if (!(rays instanceof Float64Array) || rays.length === 0 || rays.length % 6 !== 0) {
    throw new TypeError(who + ': rays must be a non-empty Float64Array of 6 numbers per ray');
  }
  const o = opts || {}, n = rays.length / 6;
  for (const name of ['pix', 'path']) {
    if (o[name] != null && !(o[name] instanceof Uint32Array && o[name].length === n)) throw new TypeError(who + ': ' + name + ' must be a Uint32Array of one element per ray');
  }
  const tail = relight ? softOf({soft: {samples: o.samples, lightRadius: o.lightRadius, offsets: o.offsets, stride: o.stride, base: o.base}}, who, true).tail : [];
  if (!inited) init(o.maxDevices);
  const r = (relight ? native().relightRays : native().shadeRays)(new Uint8Array(flattenScene(sceneObj)), rays, o.pix || null, o.path || null, !!o.bin, ...tail);
  r.node = (i) => {
    if (!Number.isInteger(i) || i < 0 || i >= r.count) throw new RangeError('node index out of range');
    return nodeAt(r.nodes, i, sceneObj);
  };
  return r;
}

// The segments of the reference's light loop (main.js:286-292) from `points` (Float64Array, 3 per point: hit.p) to every light of the
// scene, operation for operation: shadow_vec = between3D(hit.p, light), light_mag = mag3D, light_len = sqrt(light_mag), scale3D by
// 1 / light_len where light_len != 0, shadow_dot = dot3D(shadow_vec, hit.l) with hit.l from `facing` (Float64Array, 3 per point, or
// null).  `skip` (Int32Array, hit_i per point, or null) is handed through.  Returns one record per light: {rays: Float64Array 6 per
// point {point, shadow_vec} as occlusion takes them, length (light_len), lightMag, shadowDot (null without facing), mask: Uint8Array
// (shadow_dot > 0: the surface faces the light; all 1 without facing), skip}.
function lightSegments(sceneObj, points, facing, skip) {
  if (!(points instanceof Float64Array) || points.length % 3 !== 0) throw new TypeError('lightSegments: points must be a Float64Array of 3 numbers per point');
  const n = points.length / 3;
  if (facing != null && !(facing instanceof Float64Array && facing.length === 3 * n)) throw new TypeError('lightSegments: facing must be a Float64Array of 3 numbers per point, or null');
  if (skip != null && !(skip instanceof Int32Array && skip.length === n)) throw new TypeError('lightSegments: skip must be an Int32Array of one index per point, or null');
  return sceneObj.lights.map((light) => {
    const rays = new Float64Array(6 * n), length = new Float64Array(n), lightMag = new Float64Array(n);
    const shadowDot = facing != null ? new Float64Array(n) : null, mask = new Uint8Array(n).fill(1);
    for (let i = 0; i < n; i++) {
      let v = [light[0] - points[3 * i], light[1] - points[3 * i + 1], light[2] - points[3 * i + 2]];
      const mag = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], len = Math.sqrt(mag);
      if (len !== 0) { const k = 1 / len; v = [v[0] * k, v[1] * k, v[2] * k]; }
      for (let c = 0; c < 3; c++) { rays[6 * i + c] = points[3 * i + c]; rays[6 * i + 3 + c] = v[c]; }
      length[i] = len; lightMag[i] = mag;
      if (shadowDot) {
        shadowDot[i] = v[0] * facing[3 * i] + v[1] * facing[3 * i + 1] + v[2] * facing[3 * i + 2];
        mask[i] = shadowDot[i] > 0 ? 1 : 0;
      }
    }
    return {rays, length, lightMag, shadowDot, mask, skip: skip != null ? skip : null};
  });
}

// The reference's shadow scan (main.js:293-304) for a list of segments: `rays` is a Float64Array of 6 numbers per ray {org, dir},
// directions used as given (lightSegments builds the reference's).  opts, one element per ray each: length (Float64Array, light_len;
// default Infinity), intensity (Float64Array, what the scan starts with; default the scene's light_intensity), skip (Int32Array, hit_i:
// the sphere left out; default none).  The scan walks scene.objects in order: a sphere met before `length` divides the intensity by its
// albedo[4], or - albedo[4] == 0 - zeroes it, becomes the blocker and ends the scan.  Returns {intensity: Float64Array, blocker:
// Int32Array (-1 = none; null unless opts.blocker)}.  A ray with a non-finite component is not traced: NaN, -1.  opts.bin: the GPU
// orders each chunk of 2^18 rays first (rt_occlusion_binned) - the same results.
function occlusion(sceneObj, rays, opts) {
  if (!(rays instanceof Float64Array) || rays.length === 0 || rays.length % 6 !== 0) {
    throw new TypeError('occlusion: rays must be a non-empty Float64Array of 6 numbers per ray');
  }
  const o = opts || {}, n = rays.length / 6;
  for (const [name, kind] of [['length', Float64Array], ['intensity', Float64Array], ['skip', Int32Array]]) {
    if (o[name] != null && !(o[name] instanceof kind && o[name].length === n)) throw new TypeError('occlusion: ' + name + ' must be a ' + kind.name + ' of one element per ray');
  }
  if (!inited) init(o.maxDevices);
  return native().occlusion(new Uint8Array(flattenScene(sceneObj)), rays, o.length || null, o.intensity || null, o.skip || null, !!o.blocker, !!o.bin);
}

// Ambient occlusion (include/rt_hip.h: struct rt_ambient): per receiver - a hit record, as traceRays / traceView return them with
// {hits: true} - opts.samples shadow scans of length opts.radius over the hemisphere of its facing normal, the receiver's own sphere left
// out, counted and averaged on the GPU.  Returns {open: Float64Array (the share of scans no opaque sphere ended; a miss: 1), intensity:
// Float64Array (their mean intensity from 1.0; glass divides by albedo[4], so it can exceed 1; NaN for a miss), rgba: Uint8ClampedArray
// (open as a grey pixel), kernel_ms} - each null unless asked for: opts.open (default true), opts.intensity, opts.rgba.
//   ambientDirs(n)                 the library's cosine-weighted spiral: Float64Array, 3 per entry, local directions with z along the normal
//   ambient(scene, hits, opts)     hits: an array of hit objects (null: a miss) or a Uint8Array of 80-byte rt_hit records.  opts: samples
//                                  (default 16), radius (default Infinity: sky visibility), dirs (default ambientDirs(samples)), stride
//                                  (default 1) and base (default 0): sample s of receiver i reads entry ((base + i) stride + s) % n_dirs
//   ambientView(scene, view, w, h, opts)   the same for what the view sees, pixel y w + x being receiver y w + x; rays, hit records and
//                                  scans stay on the GPU.  opts.rgba defaults to true and opts.open to false here.
const HIT_BYTES = 80;
function hitRecords(hits) {
  if (hits instanceof Uint8Array) return hits;
  const buf = new Uint8Array(HIT_BYTES * hits.length), d = new DataView(buf.buffer);
  hits.forEach((h, i) => {
    const at = HIT_BYTES * i;
    if (!h) { d.setInt32(at, -1, true); d.setFloat64(at + 8, Infinity, true); return; }
    d.setInt32(at, h.index, true); d.setInt32(at + 4, h.inside ? 1 : 0, true); d.setFloat64(at + 8, h.t, true);
    for (let c = 0; c < 3; c++) { d.setFloat64(at + 16 + 8 * c, h.point[c], true); d.setFloat64(at + 40 + 8 * c, h.normal[c], true); }
    d.setFloat64(at + 64, h.u, true); d.setFloat64(at + 72, h.v, true);
  });
  return buf;
}
function ambientDirs(n) { return native().ambientDirs(n); }
function ambientOpts(o, who) {
  const samples = o.samples === undefined ? 16 : o.samples, dirs = o.dirs || native().ambientDirs(samples);
  if (!(dirs instanceof Float64Array) || dirs.length === 0 || dirs.length % 3 !== 0) throw new TypeError(who + ': dirs must be a Float64Array of 3 numbers per direction');
  return [dirs, samples, o.stride === undefined ? 1 : o.stride, o.base || 0, o.radius === undefined ? Infinity : o.radius];
}
function ambient(sceneObj, hits, opts) {
  if (!(hits instanceof Uint8Array ? hits.length > 0 && hits.length % HIT_BYTES === 0 : Array.isArray(hits) && hits.length > 0)) {
    throw new TypeError('ambient: hits must be a non-empty array of hit objects or a Uint8Array of 80-byte records');
  }
  const o = opts || {};
  const args = ambientOpts(o, 'ambient');
  if (!inited) init(o.maxDevices);
  return native().ambient(new Uint8Array(flattenScene(sceneObj)), hitRecords(hits), ...args, o.open !== false, !!o.intensity, !!o.rgba);
}
function ambientView(sceneObj, view, w, h, opts) {
  if (!view || !Number.isInteger(view.model)) throw new TypeError('ambientView: view must come from views.reference / pinhole / ortho / equirect');
  const o = opts || {};
  const args = ambientOpts(o, 'ambientView');
  if (!inited) init(o.maxDevices);
  return native().ambientView(new Uint8Array(flattenScene(sceneObj)), viewBytes(view), view.lon || null, view.lat || null, w, h, ...args,
    !!o.open, !!o.intensity, o.rgba !== false);
}

// Gathered light (include/rt_hip.h: struct rt_gather): what colour arrives at each receiver from the rest of the scene - opts.samples rays
// over the hemisphere of its facing normal along the directions ambient uses, each traced as traceRays traces any ray (depth opts.segs,
// 0 = the scene's; no sphere left out), averaged on the GPU in one launch.  With the default cosine-weighted table rgb is irradiance / pi.
// Returns {rgb: Float64Array (3 per receiver; NaN for a miss), rgba: Uint8ClampedArray (the mean as a pixel), kernel_ms} - each null
// unless named in opts.want.
//   gather(scene, hits, opts)      hits as for ambient.  opts: samples (default 16), dirs (default ambientDirs(samples)), stride (default 1),
//                                  segs (default 0), base and pixBase (default 0), pixStride (default: the number of receivers; the stars
//                                  sampler's pix of sample s of receiver i is pixBase + s pixStride + i), want (default ['rgb'])
//   gatherView(scene, view, w, h, opts)   the same for what the view sees; pixStride defaults to w h, want to ['rgba']
//   gather(..., {mapping: 'samples'})   the same bytes from the probe call (rt_gather_probes): one workgroup per receiver, its samples on
//                                  lanes - for SHORT lists (light probes); the default mapping 'receivers' is the call above.  With
//                                  opts.weights (Float64Array, one row of 1..16 numbers per table entry) want may name 'coef':
//                                  Float64Array, per receiver, weight k and channel the mean of weights[e_s][k] c_s, e_s being the entry
//                                  sample s took its direction from
//   sh9Weights(dirs)               nine real spherical-harmonics values per direction, in the header's order: a weight table
//   probes(scene, points, opts)    light probes at points in free space ([x, y, z] each): gather with mapping 'samples', stride 0 and
//                                  hand-made records (normal [0, 0, 1], object 0: table directions are world directions).  opts: samples
//                                  (default 64), dirs (default lightingOffsets(samples): the whole sphere), weights, segs, pixBase, want
const GATHER_OUTPUTS = ['rgb', 'rgba'];
function gatherOpts(o, who, n, wantDefault, outputs) {
  const names = outputs || GATHER_OUTPUTS;
  const samples = o.samples === undefined ? 16 : o.samples, dirs = o.dirs || native().ambientDirs(samples);
  if (!(dirs instanceof Float64Array) || dirs.length === 0 || dirs.length % 3 !== 0) throw new TypeError(who + ': dirs must be a Float64Array of 3 numbers per direction');
  const want = o.want === undefined ? wantDefault : o.want;
  if (!Array.isArray(want) || want.length === 0 || !want.every((k) => names.includes(k))) throw new TypeError(who + ': want names some of ' + names.map((k) => "'" + k + "'").join(', '));
  return [dirs, samples, o.stride === undefined ? 1 : o.stride, o.segs || 0, o.base || 0, o.pixBase || 0, o.pixStride === undefined ? n : o.pixStride,
    ...names.map((k) => want.includes(k))];
}
function gather(sceneObj, hits, opts) {
  if (!(hits instanceof Uint8Array ? hits.length > 0 && hits.length % HIT_BYTES === 0 : Array.isArray(hits) && hits.length > 0)) {
    throw new TypeError('gather: hits must be a non-empty array of hit objects or a Uint8Array of 80-byte records');
  }
  const o = opts || {}, n = hits instanceof Uint8Array ? hits.length / HIT_BYTES : hits.length;
  const mapping = o.mapping === undefined ? 'receivers' : o.mapping;
  if (mapping !== 'receivers' && mapping !== 'samples') throw new TypeError("gather: mapping is 'receivers' or 'samples'");
  if (o.weights != null && mapping !== 'samples') throw new TypeError("gather: weights need mapping 'samples'");
  if (mapping === 'receivers') {
    const args = gatherOpts(o, 'gather', n, ['rgb']);
    if (!inited) init(o.maxDevices);
    return native().gather(new Uint8Array(flattenScene(sceneObj)), hitRecords(hits), ...args);
  }
  const w = o.weights == null ? null : o.weights;
  const args = gatherOpts(o, 'gather', n, ['rgb'], w ? ['rgb', 'rgba', 'coef'] : GATHER_OUTPUTS), nDirs = args[0].length / 3;
  if (w && !(w instanceof Float64Array && w.length > 0 && w.length % nDirs === 0 && w.length / nDirs <= 16)) {
    throw new TypeError('gather: weights must be a Float64Array of 1..16 numbers per table entry');
  }
  if (w && !args[9]) throw new TypeError("gather: weights are given: want names 'coef'");
  if (!inited) init(o.maxDevices);
  return native().gatherProbes(new Uint8Array(flattenScene(sceneObj)), hitRecords(hits), args[0], w, w ? w.length / nDirs : 0, ...args.slice(1, 9), w ? args[9] : false);
}
function sh9Weights(dirs) { return native().sh9Weights(dirs); }
function probes(sceneObj, points, opts) {
  if (!Array.isArray(points) || points.length === 0 || !points.every((p) => p && p.length === 3)) throw new TypeError('probes: points must be a non-empty array of [x, y, z]');
  const o = opts || {}, samples = o.samples === undefined ? 64 : o.samples;
  const recs = points.map((p) => ({index: 0, inside: false, t: 0, point: p, normal: [0, 0, 1], u: 0, v: 0}));
  return gather(sceneObj, recs, {samples, dirs: o.dirs || native().lightingOffsets(samples), weights: o.weights, segs: o.segs, pixBase: o.pixBase, stride: 0,
    mapping: 'samples', want: o.want, maxDevices: o.maxDevices});
}
function gatherView(sceneObj, view, w, h, opts) {
  if (!view || !Number.isInteger(view.model)) throw new TypeError('gatherView: view must come from views.reference / pinhole / ortho / equirect');
  const o = opts || {};
  const args = gatherOpts(o, 'gatherView', w * h, ['rgba']);
  if (!inited) init(o.maxDevices);
  return native().gatherView(new Uint8Array(flattenScene(sceneObj)), viewBytes(view), view.lon || null, view.lat || null, w, h, ...args);
}

// Sampled lights (include/rt_hip.h: struct rt_lighting): how much light arrives at each receiver - the reference's light loop
// (main.js:283-306) opts.samples times, every light displaced by opts.lightRadius times an entry of opts.offsets, averaged on the GPU.
// With the defaults (one sample, lightRadius 0) it is the reference's own loop.  Returns {diffuse: Float64Array (the mean raw diffuse
// sum), intensity: Float64Array (the mean intensity left after the last light, quirk q2), lit: Float64Array (the share of (sample, light)
// pairs that arrived), rgba: Uint8ClampedArray (min(1, diffuse) as a grey pixel), kernel_ms} - each null unless named in opts.want.
//   lightingOffsets(n)             the library's spiral over the unit sphere: Float64Array, 3 per entry
//   lighting(scene, hits, opts)    hits as for ambient.  opts: samples (default 1), lightRadius (default 0), offsets (default
//                                  lightingOffsets(samples)), stride (default 1), base (default 0), want (default ['diffuse'])
//   lightingView(scene, view, w, h, opts)   the same for what the view sees; want defaults to ['rgba']
const LIGHTING_OUTPUTS = ['diffuse', 'intensity', 'lit', 'rgba'];
function lightingOffsets(n) { return native().lightingOffsets(n); }
function lightingOpts(o, who, wantDefault) {
  const samples = o.samples === undefined ? 1 : o.samples, offs = o.offsets || native().lightingOffsets(samples);
  if (!(offs instanceof Float64Array) || offs.length === 0 || offs.length % 3 !== 0) throw new TypeError(who + ': offsets must be a Float64Array of 3 numbers per entry');
  const want = o.want === undefined ? wantDefault : o.want;
  if (!Array.isArray(want) || want.length === 0 || !want.every((k) => LIGHTING_OUTPUTS.includes(k))) {
    throw new TypeError(who + ": want names some of 'diffuse', 'intensity', 'lit', 'rgba'");
  }
  return [offs, samples, o.stride === undefined ? 1 : o.stride, o.base || 0, o.lightRadius === undefined ? 0 : o.lightRadius,
    ...LIGHTING_OUTPUTS.map((k) => want.includes(k))];
}
function lighting(sceneObj, hits, opts) {
  if (!(hits instanceof Uint8Array ? hits.length > 0 && hits.length % HIT_BYTES === 0 : Array.isArray(hits) && hits.length > 0)) {
    throw new TypeError('lighting: hits must be a non-empty array of hit objects or a Uint8Array of 80-byte records');
  }
  const o = opts || {};
  const args = lightingOpts(o, 'lighting', ['diffuse']);
  if (!inited) init(o.maxDevices);
  return native().lighting(new Uint8Array(flattenScene(sceneObj)), hitRecords(hits), ...args);
}
function lightingView(sceneObj, view, w, h, opts) {
  if (!view || !Number.isInteger(view.model)) throw new TypeError('lightingView: view must come from views.reference / pinhole / ortho / equirect');
  const o = opts || {};
  const args = lightingOpts(o, 'lightingView', ['rgba']);
  if (!inited) init(o.maxDevices);
  return native().lightingView(new Uint8Array(flattenScene(sceneObj)), viewBytes(view), view.lon || null, view.lat || null, w, h, ...args);
}

// `const build = '741'` (main.js:3) + this library's revision; every render's `.stats` also carries `.build` and `.report`, the
// reference's end-of-frame string 'build #<id> (<elapsed>ms)' (main.js:204-205) for that render.
function buildId() { return native().buildId(); }

function shutdown() { if (addon) addon.shutdown(); inited = false; }

module.exports = Object.assign({render, renderAsync, renderProgressive, renderHits, pick, traceRays, traceView, views, shadeRays, relightRays, primaryRays, normal3D, occlusion, lightSegments, ambient, ambientView, ambientDirs, gather, gatherView, sh9Weights, probes, lighting, lightingView, lightingOffsets, init, shutdown, buildId, flattenScene, scenes, native}, scene);
