'use strict';
// Driven by tests/test_gpu_node_occlusion.py: RT.lightSegments + RT.occlusion run the reference's light loop (main.js:283-305) over
// the given nodes - one intensity carried from light to light - with and without {bin: true}.
//   node js_occlusion_check.js <package dir> <scene name> <base64 points> <base64 facing> <base64 skip>
const [pkg, name, p64, f64, s64] = process.argv.slice(2);
const fs = require('fs'), path = require('path');
const RT = require(path.join(pkg, 'js', 'index.js')), F = require(path.join(pkg, 'js', 'flatten.js'));
const scene = F.sceneFromJSON(fs.readFileSync(path.join(pkg, 'scenes', name + '.json'), 'utf8'), path.join(pkg, 'scenes'));
const slice = (s) => { const b = Buffer.from(s, 'base64'); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const points = new Float64Array(slice(p64)), facing = new Float64Array(slice(f64)), skip = new Int32Array(slice(s64));
const n = skip.length;
const raw = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
function lightLoop(bin) {
  const li = new Float64Array(n).fill(scene.light_intensity === undefined ? 50 : scene.light_intensity);
  const blockers = [];
  for (const g of RT.lightSegments(scene, points, facing, skip)) {
    const idx = [];
    for (let i = 0; i < n; i++) if (g.mask[i]) idx.push(i);
    if (idx.length === 0) continue;
    const rays = new Float64Array(6 * idx.length), length = new Float64Array(idx.length), intensity = new Float64Array(idx.length), sk = new Int32Array(idx.length);
    idx.forEach((i, j) => { rays.set(g.rays.subarray(6 * i, 6 * i + 6), 6 * j); length[j] = g.length[i]; intensity[j] = li[i]; sk[j] = skip[i]; });
    const r = RT.occlusion(scene, rays, {length, intensity, skip: sk, blocker: true, bin});
    idx.forEach((i, j) => { li[i] = r.intensity[j]; });
    blockers.push(Array.from(r.blocker));
  }
  return {li, blockers};
}
const plain = lightLoop(false), binned = lightLoop(true);
const bare = RT.occlusion(scene, new Float64Array([0, 1.5, 10, 0, 0, -1, 0, NaN, 10, 0, 0, -1]));
RT.shutdown();
console.log(JSON.stringify({intensity: raw(plain.li).toString('base64'), blockers: plain.blockers,
  same: raw(plain.li).equals(raw(binned.li)) && JSON.stringify(plain.blockers) === JSON.stringify(binned.blockers),
  bare: [bare.blocker, Number.isNaN(bare.intensity[1]), bare.intensity.length]}));
