// js_view_samples_check - sampled views from Node for tests/test_node_view_samples.py:
//   node js_view_samples_check.js <package dir> pattern            the k = 1..4 grids and a lens, as the library gives them
//   node js_view_samples_check.js <package dir> trace <w> <h>      RT.traceView with {samples: sampleGrid(2), lens} and without either option
// prints one line of JSON; binary data is base64.
const pkg = process.argv[2], what = process.argv[3];
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const b64 = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64');
const flat = (samples) => b64(Float64Array.from(samples.flatMap((s) => [s.dx, s.dy, s.lu, s.lv])));
const cam = JSON.parse(process.env.RT_CHECK_CAM), eye = JSON.parse(process.env.RT_CHECK_EYE);

if (what === 'pattern') {
  console.log(JSON.stringify({grids: [1, 2, 3, 4].map((k) => flat(RT.views.sampleGrid(k))), lens: RT.views.lens(0.07, 6.5)}));
} else {
  const w = Number(process.argv[4]), h = Number(process.argv[5]);
  const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14.json', 'utf8'), pkg + '/scenes');
  const samples = RT.views.sampleGrid(2), lens = RT.views.lens(0.07, 6.5);
  const a = RT.traceView(sc, RT.views.pinhole(...cam, 52), w, h, {samples, lens, rgb: true});
  const b = RT.traceView(sc, RT.views.equirect(...eye, w, h), w, h, {samples});
  const c = RT.traceView(sc, RT.views.pinhole(...cam, 52), w, h, {lens: RT.views.lens(0, 1)});       // no samples: the zero sample; radius 0: no lens
  const plain = RT.traceView(sc, RT.views.pinhole(...cam, 52), w, h);
  let refused = null;
  try { RT.traceView(sc, RT.views.pinhole(...cam, 52), w, h, {samples, hits: true}); } catch (e) { refused = e.constructor.name; }
  console.log(JSON.stringify({pinhole: {rgba: b64(a.rgba), rgb: b64(a.rgb), type: Object.prototype.toString.call(a.rgba), hits: a.hits},
    equirect: {rgba: b64(b.rgba), rgb: b.rgb}, zero: b64(c.rgba), plain: b64(plain.rgba), plainHits: plain.hits, refused}));
}
