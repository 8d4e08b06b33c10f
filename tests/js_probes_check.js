// js_probes_check - probes from Node for tests/test_gpu_probes.py:
//   node js_probes_check.js <package dir> <reference.json>
// The reference holds what Python's host forms gave (base64): hits (the receivers), rgb, rgba and coef of
// rt_host.gather(default14, hits, 65, dirs=ambient_dirs(128), stride=7, segs=2, mapping="samples", weights=sh9_weights(dirs)), sh9 (those
// weights), points, probe_rgb and probe_coef of rt_host.probes(default14, points, 64, weights=sh9_weights(lighting_offsets(64))).
// Prints one line of JSON: per output whether Node's bytes are Python's, and what RT.gather refuses before any library call.
const pkg = process.argv[2], ref = JSON.parse(require('fs').readFileSync(process.argv[3], 'utf8'));
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14.json', 'utf8'), pkg + '/scenes');
const same = (a, b64) => a !== null && Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b64, 'base64'));
const name = (f) => { try { f(); return null; } catch (e) { return e.constructor.name; } };

const hits = new Uint8Array(Buffer.from(ref.hits, 'base64'));
const dirs = RT.ambientDirs(128), weights = RT.sh9Weights(dirs);
const refused = [name(() => RT.gather(sc, hits, {mapping: 'bogus'})), name(() => RT.gather(sc, hits, {weights})),
  name(() => RT.gather(sc, hits, {mapping: 'samples', want: ['coef']}))];
const g = RT.gather(sc, hits, {samples: 65, dirs, stride: 7, segs: 2, mapping: 'samples', weights, want: ['rgb', 'rgba', 'coef']});
const sphere = RT.lightingOffsets(64);
const p = RT.probes(sc, ref.points, {samples: 64, weights: RT.sh9Weights(sphere), want: ['rgb', 'coef']});
console.log(JSON.stringify({rgb: same(g.rgb, ref.rgb), rgba: same(g.rgba, ref.rgba), coef: same(g.coef, ref.coef), sh9: same(weights, ref.sh9),
  probe_rgb: same(p.rgb, ref.probe_rgb), probe_coef: same(p.coef, ref.probe_coef), refused}));
