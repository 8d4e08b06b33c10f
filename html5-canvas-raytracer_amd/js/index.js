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
function render(width, height, sceneObj, opts) {
  if (!inited) init(opts && opts.maxDevices);
  const r = native().render(flattenScene(sceneObj), width, height, flagsOf(opts), (opts && opts.into) || undefined);
  r.data.stats = r.stats;
  return r.data;
}

// Promise variant: the launch and the copy-out run off the event loop (napi_async_work)
function renderAsync(width, height, sceneObj, opts) {
  try { if (!inited) init(opts && opts.maxDevices); } catch (e) { return Promise.reject(e); }
  return native().renderAsync(flattenScene(sceneObj), width, height, flagsOf(opts)).then((r) => { r.data.stats = r.stats; return r.data; });
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
function traceRays(sceneObj, rays, opts) {
  if (!(rays instanceof Float64Array) || rays.length === 0 || rays.length % 6 !== 0) {
    throw new TypeError('traceRays: rays must be a non-empty Float64Array of 6 numbers per ray');
  }
  if (!inited) init(opts && opts.maxDevices);
  const o = opts || {};
  const r = native().traceRays(new Uint8Array(flattenScene(sceneObj)), rays, o.segs || 0, o.rgb !== false, !!o.rgba, !!o.hits, !!o.bin);
  if (r.hits) for (const h of r.hits) if (h) h.object = sceneObj.objects[h.index];
  return r;
}

// `const build = '741'` (main.js:3) + this library's revision; every render's `.stats` also carries `.build` and `.report`, the
// reference's end-of-frame string 'build #<id> (<elapsed>ms)' (main.js:204-205) for that render.
function buildId() { return native().buildId(); }

function shutdown() { if (addon) addon.shutdown(); inited = false; }

module.exports = Object.assign({render, renderAsync, renderProgressive, renderHits, pick, traceRays, primaryRays, normal3D, init, shutdown, buildId, flattenScene, scenes, native}, scene);
