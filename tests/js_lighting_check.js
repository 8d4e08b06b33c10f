// js_lighting_check - sampled lights from Node for tests/test_node_lighting.py:
//   node js_lighting_check.js <package dir> offsets                RT.lightingOffsets(n) for n = 1, 16, 64, as the library gives them
//   node js_lighting_check.js <package dir> lighting <w> <h>       RT.traceView's hit objects fed to RT.lighting, the list in two pieces with
//                                                                  base, and RT.lightingView of the same view (default14, the scene's camera)
// prints one line of JSON; binary data is base64.
const pkg = process.argv[2], what = process.argv[3];
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const b64 = (a) => (a ? Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64') : null);
const KEYS = ['diffuse', 'intensity', 'lit', 'rgba'];
const all = (r) => Object.fromEntries(KEYS.map((k) => [k, b64(r[k])]));

if (what === 'offsets') {
  console.log(JSON.stringify({offsets: [1, 16, 64].map((n) => b64(RT.lightingOffsets(n)))}));
} else {
  const w = Number(process.argv[4]), h = Number(process.argv[5]);
  const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14.json', 'utf8'), pkg + '/scenes');
  const c = sc.camera, view = RT.views.pinhole(c.origin, c.axisX, c.axisY, c.axisZ, sc.fovDeg);
  const hits = RT.traceView(sc, view, w, h, {hits: true, rgba: false}).hits;
  const opts = {samples: 5, lightRadius: 1, offsets: RT.lightingOffsets(64), stride: 7, want: KEYS};
  const a = RT.lighting(sc, hits, opts);
  const pieces = [0, 100].map((at) => RT.lighting(sc, hits.slice(at, at ? hits.length : 100), Object.assign({}, opts, {base: at})));   // a list in two pieces, with base
  const v = RT.lightingView(sc, view, w, h, opts);
  const plain = RT.lighting(sc, hits.slice(0, 50));                // the defaults: the reference's own loop, diffuse only
  const picture = RT.lightingView(sc, view, w, h, {samples: 5, lightRadius: 1});   // ... and a view's: the picture only
  const refused = [];
  for (const f of [() => RT.lighting(sc, []), () => RT.lighting(sc, hits, {want: ['colour']}), () => RT.lighting(sc, hits, {offsets: [0, 0, 1]})]) {
    try { f(); refused.push(null); } catch (e) { refused.push(e.constructor.name); }
  }
  console.log(JSON.stringify({list: Object.assign(all(a), {type: Object.prototype.toString.call(a.rgba)}), pieces: pieces.map(all), view: all(v),
    plain: {diffuse: b64(plain.diffuse), intensity: plain.intensity, lit: plain.lit, rgba: plain.rgba},
    picture: {diffuse: picture.diffuse, intensity: picture.intensity, lit: picture.lit, rgba: b64(picture.rgba)}, refused}));
}
