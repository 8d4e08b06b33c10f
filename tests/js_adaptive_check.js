'use strict';
// Driven by tests/test_gpu_adaptive.py: RT.render and RT.renderAsync with {adaptive: {k, threshold}}, with and without opts.into.
//   node js_adaptive_check.js <package dir> <scene name> <width> <height> <k> <threshold>
const [pkg, name, ws, hs, ks, ts] = process.argv.slice(2);
const fs = require('fs'), path = require('path');
const RT = require(path.join(pkg, 'js', 'index.js')), F = require(path.join(pkg, 'js', 'flatten.js'));
const scene = F.sceneFromJSON(fs.readFileSync(path.join(pkg, 'scenes', name + '.json'), 'utf8'), path.join(pkg, 'scenes'));
const w = +ws, h = +hs, adaptive = {k: +ks, threshold: +ts};
const raw = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const plain = RT.render(w, h, scene);
const sync = RT.render(w, h, scene, {adaptive});
const mine = new Uint8ClampedArray(4 * w * h);
const into = RT.render(w, h, scene, {adaptive, into: mine});
const bad = [];
for (const f of [() => RT.render(w, h, scene, {adaptive: {k: 5, threshold: 32}}), () => RT.render(w, h, scene, {adaptive: {k: 2, threshold: 257}})]) {
  try { f(); bad.push(false); } catch (e) { bad.push(e instanceof Error); }
}
RT.renderAsync(w, h, scene, {adaptive}).then((later) => {
  RT.shutdown();
  console.log(JSON.stringify({frame: raw(sync).toString('base64'), refined: sync.stats.refined, pixels: sync.stats.pixels, plain: raw(plain).toString('base64'),
    plainRefined: plain.stats.refined === undefined, into: into === mine && raw(mine).equals(raw(sync)) && into.stats.refined === sync.stats.refined,
    later: raw(later).equals(raw(sync)) && later.stats.refined === sync.stats.refined, bad}));
}, (e) => { console.error(e); process.exit(1); });
