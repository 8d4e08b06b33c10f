// js_ambient_check - ambient occlusion from Node for tests/test_node_ambient.py:
//   node js_ambient_check.js <package dir> dirs                 RT.ambientDirs(n) for n = 1, 16, 64, as the library gives them
//   node js_ambient_check.js <package dir> ambient <w> <h>      RT.traceView's hit objects fed to RT.ambient, the same receivers as 80-byte
//                                                               records, and RT.ambientView of the same view (default14, the scene's camera)
// prints one line of JSON; binary data is base64.
const pkg = process.argv[2], what = process.argv[3];
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const b64 = (a) => (a ? Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64') : null);

if (what === 'dirs') {
  console.log(JSON.stringify({dirs: [1, 16, 64].map((n) => b64(RT.ambientDirs(n)))}));
} else {
  const w = Number(process.argv[4]), h = Number(process.argv[5]);
  const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14.json', 'utf8'), pkg + '/scenes');
  const c = sc.camera, view = RT.views.pinhole(c.origin, c.axisX, c.axisY, c.axisZ, sc.fovDeg);
  const hits = RT.traceView(sc, view, w, h, {hits: true, rgba: false}).hits;
  const opts = {samples: 5, radius: 2, dirs: RT.ambientDirs(64), stride: 7, open: true, intensity: true, rgba: true};
  const a = RT.ambient(sc, hits, opts);
  const pieces = [0, 100].map((at) => RT.ambient(sc, hits.slice(at, at ? hits.length : 100), Object.assign({}, opts, {base: at})));   // a list in two pieces, with base
  const v = RT.ambientView(sc, view, w, h, opts);
  const plain = RT.ambient(sc, hits.slice(0, 50));                 // the defaults: 16 samples of the library's table, radius Infinity, open only
  const picture = RT.ambientView(sc, view, w, h, {samples: 5, radius: 2});   // ... and a view's: the picture only
  let refused = null;
  try { RT.ambient(sc, []); } catch (e) { refused = e.constructor.name; }
  console.log(JSON.stringify({list: {open: b64(a.open), intensity: b64(a.intensity), rgba: b64(a.rgba), type: Object.prototype.toString.call(a.rgba)},
    pieces: pieces.map((q) => ({open: b64(q.open), intensity: b64(q.intensity), rgba: b64(q.rgba)})),
    view: {open: b64(v.open), intensity: b64(v.intensity), rgba: b64(v.rgba)},
    plain: {open: b64(plain.open), intensity: plain.intensity, rgba: plain.rgba},
    picture: {open: picture.open, intensity: picture.intensity, rgba: b64(picture.rgba)}, refused}));
}
