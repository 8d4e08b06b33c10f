'use strict';
// Driven by tests/test_gpu_nodes.py: RT.shadeRays (one level of intersectWorld) with and without pix / path and {bin: true}, its
// node(i) accessor, and RT.traceRays {wavefront: true} against the recursive RT.traceRays.
//   node js_nodes_check.js <package dir> <scene name> <base64 rays> <base64 pix> <base64 path>
const [pkg, name, r64, p64, t64] = process.argv.slice(2);
const fs = require('fs'), path = require('path');
const RT = require(path.join(pkg, 'js', 'index.js')), F = require(path.join(pkg, 'js', 'flatten.js'));
const scene = F.sceneFromJSON(fs.readFileSync(path.join(pkg, 'scenes', name + '.json'), 'utf8'), path.join(pkg, 'scenes'));
const slice = (s) => { const b = Buffer.from(s, 'base64'); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const rays = new Float64Array(slice(r64)), pix = new Uint32Array(slice(p64)), pth = new Uint32Array(slice(t64));
const b64 = (ab) => Buffer.from(ab).toString('base64');
const raw = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const plain = RT.shadeRays(scene, rays), binned = RT.shadeRays(scene, rays, {bin: true}), tagged = RT.shadeRays(scene, rays, {pix, path: pth});
const nodes = [];
for (let i = 0; i < plain.count; i++) { const nd = plain.node(i); if (nd.hit) delete nd.hit.object; nodes.push(nd); }
const rec = RT.traceRays(scene, rays, {rgb: true, rgba: true}), wave = RT.traceRays(scene, rays, {rgb: true, rgba: true, wavefront: true});
const ordered = RT.traceRays(scene, rays, {rgb: true, wavefront: true, orderLevels: true});
const bad = [];
for (const f of [() => RT.shadeRays(scene, new Float64Array(5)), () => RT.shadeRays(scene, rays, {pix: new Uint32Array(1)}),
  () => RT.traceRays(scene, rays, {wavefront: true, hits: true}), () => plain.node(plain.count)]) {
  try { f(); bad.push(false); } catch (e) { bad.push(e instanceof TypeError || e instanceof RangeError); }
}
RT.shutdown();
console.log(JSON.stringify({count: plain.count, nodes: b64(plain.nodes), binned: Buffer.from(plain.nodes).equals(Buffer.from(binned.nodes)),
  tagged: b64(tagged.nodes), accessor: nodes, sameRgb: raw(rec.rgb).equals(raw(wave.rgb)) && raw(rec.rgb).equals(raw(ordered.rgb)),
  sameRgba: raw(rec.rgba).equals(raw(wave.rgba)), rgb: raw(wave.rgb).toString('base64'), levelCounts: wave.levelCounts, bad}));
