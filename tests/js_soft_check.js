// js_soft_check - the soft trace in one launch from Node for tests/test_node_soft.py:
//   node js_soft_check.js <package dir> <w> <h>     default14's primary rays at w x h: RT.traceRays(..., {soft}) by both methods, the
//                                                   recursive method binned, RT.traceView(..., {soft}) of the scene's camera as a pinhole,
//                                                   and what a malformed request throws
// prints one line of JSON; binary data is base64.
const pkg = process.argv[2], w = Number(process.argv[3]), h = Number(process.argv[4]);
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const b64 = (a) => (a ? Buffer.from(a.buffer || a, a.byteOffset || 0, a.byteLength).toString('base64') : null);
const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14.json', 'utf8'), pkg + '/scenes');
const rays = RT.primaryRays(w, h, sc);
const offsets = RT.lightingOffsets(8);
const soft = {samples: 4, lightRadius: 1, offsets, stride: 1, levels: 2, base: 3};
const want = {rgb: true, rgba: true};
const wavefront = RT.traceRays(sc, rays, Object.assign({soft}, want));
const named = RT.traceRays(sc, rays, Object.assign({soft: Object.assign({method: 'wavefront'}, soft)}, want));
const recursive = RT.traceRays(sc, rays, Object.assign({soft: Object.assign({method: 'recursive'}, soft)}, want));
const binned = RT.traceRays(sc, rays, Object.assign({soft: Object.assign({method: 'recursive'}, soft), bin: true}, want));
const c = sc.camera;
const view = RT.views.pinhole(c.origin, c.axisX, c.axisY, c.axisZ, sc.fovDeg);
const vsoft = {samples: 4, lightRadius: 1, offsets, stride: 1, levels: 2};
const viewSoft = RT.traceView(sc, view, w, h, Object.assign({soft: vsoft}, want));
const viewHard = RT.traceView(sc, view, w, h, want);
const refused = [];
const tries = [
  () => RT.traceRays(sc, rays, {soft: Object.assign({method: 'fast'}, soft)}),
  () => RT.traceRays(sc, rays, {soft: Object.assign({method: 'recursive'}, soft), hits: true}),
  () => RT.traceRays(sc, rays, {soft: Object.assign({method: 'recursive'}, soft), wavefront: true}),
  () => RT.traceRays(sc, rays, {soft, bin: true}),
  () => RT.traceView(sc, view, w, h, {soft: vsoft, hits: true}),
  () => RT.traceView(sc, view, w, h, {soft: vsoft, samples: RT.views.sampleGrid(2)}),
  () => RT.traceView(sc, view, w, h, {soft: {samples: 0, lightRadius: 1}}),
];
for (const t of tries) { try { t(); refused.push('accepted'); } catch (e) { refused.push(e.constructor.name); } }
const pic = (r) => ({rgb: b64(r.rgb), rgba: b64(r.rgba), levelCounts: r.levelCounts === undefined ? null : r.levelCounts, type: Object.prototype.toString.call(r.rgba)});
console.log(JSON.stringify({rays: b64(rays), wavefront: pic(wavefront), named: pic(named), recursive: pic(recursive), binned: pic(binned),
  viewSoft: pic(viewSoft), viewHard: pic(viewHard), refused}));
