// js_gather_check - gathered light from Node for tests/test_node_gather.py:
//   node js_gather_check.js <package dir> refusals              what RT.gather / RT.gatherView refuse before any library call
//   node js_gather_check.js <package dir> gather <w> <h>        RT.traceView's hit objects fed to RT.gather, the same list in two pieces, and
//                                                               RT.gatherView of the same view (default14_stars, the scene's camera)
// prints one line of JSON; binary data is base64.
const pkg = process.argv[2], what = process.argv[3];
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const b64 = (a) => (a ? Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64') : null);
const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14_stars.json', 'utf8'), pkg + '/scenes');
const c = sc.camera, view = RT.views.pinhole(c.origin, c.axisX, c.axisY, c.axisZ, sc.fovDeg);
const name = (f) => { try { f(); return null; } catch (e) { return e.constructor.name; } };

if (what === 'refusals') {
  const hit = new Uint8Array(80);
  console.log(JSON.stringify({refused: [
    name(() => RT.gather(sc, [])), name(() => RT.gather(sc, new Uint8Array(81))), name(() => RT.gather(sc, hit, {want: ['open']})),
    name(() => RT.gather(sc, hit, {want: []})), name(() => RT.gather(sc, hit, {dirs: new Float64Array(4)})), name(() => RT.gatherView(sc, {}, 4, 3)),
    name(() => RT.gatherView(sc, view, 4, 3, {want: 'rgba'}))]}));
} else {
  const w = Number(process.argv[4]), h = Number(process.argv[5]);
  const hits = RT.traceView(sc, view, w, h, {hits: true, rgba: false}).hits;
  const opts = {samples: 5, dirs: RT.ambientDirs(64), stride: 7, segs: 2, want: ['rgb', 'rgba']};
  const a = RT.gather(sc, hits, opts);
  // a list in two pieces, with base and pixBase, and the whole list's pixStride
  const pieces = [0, 100].map((at) => RT.gather(sc, hits.slice(at, at ? hits.length : 100), Object.assign({}, opts, {base: at, pixBase: at, pixStride: hits.length})));
  const v = RT.gatherView(sc, view, w, h, opts);
  const flat = RT.gather(sc, hits, Object.assign({}, opts, {pixStride: 0, pixBase: 7}));
  const plain = RT.gather(sc, hits.slice(0, 50));                 // the defaults: 16 samples of the library's table, the scene's depth, rgb only
  const picture = RT.gatherView(sc, view, w, h, {samples: 5});    // ... and a view's: the picture only
  const pack = (q) => ({rgb: b64(q.rgb), rgba: b64(q.rgba)});
  console.log(JSON.stringify({list: Object.assign(pack(a), {type: Object.prototype.toString.call(a.rgba)}), pieces: pieces.map(pack), view: pack(v), flat: pack(flat),
    plain: {rgb: b64(plain.rgb), rgba: plain.rgba}, picture: {rgb: picture.rgb, rgba: b64(picture.rgba)}, kernel_ms: a.kernel_ms}));
}
