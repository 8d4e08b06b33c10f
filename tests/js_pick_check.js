'use strict';
// Driven by tests/test_gpu_hits.py: RT.renderHits / RT.pick and GET /pick on default14 at 160x90; the Python side compares.
const crypto = require('crypto');
const fs = require('fs');
const http = require('http');
const path = require('path');
const ROOT = path.join(__dirname, '..');
const PKG = path.join(ROOT, 'html5-canvas-raytracer_amd');
const RT = require(path.join(PKG, 'js', 'index.js'));
const F = require(path.join(PKG, 'js', 'flatten.js'));
const S = require(path.join(PKG, 'js', 'server.js'));
const sha = (ta) => crypto.createHash('sha256').update(Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)).digest('hex');
const get = (port, p) => new Promise((resolve, reject) => {
  http.get({host: '127.0.0.1', port, path: p}, (res) => { const c = []; res.on('data', (d) => c.push(d)); res.on('end', () => resolve({status: res.statusCode, body: Buffer.concat(c).toString()})); }).on('error', reject);
});
(async () => {
  const w = 160, h = 90;
  const scene = F.sceneFromJSON(fs.readFileSync(path.join(PKG, 'scenes', 'default14.json'), 'utf8'), path.join(PKG, 'scenes'));
  const out = {};
  const r = RT.renderHits(w, h, scene);
  out.hits = {id: sha(r.id), depth: sha(r.depth), normal: sha(r.normal), width: r.width, height: r.height};
  const o = RT.renderHits(w, h, scene, {depth: false, normal: false});
  out.idOnly = {id: sha(o.id), depth: o.depth, normal: o.normal};
  out.pixels = [[0, 0], [80, 45], [10, 80], [159, 89], [40, 60], [120, 30], [70, 70], [100, 50]];
  out.picks = out.pixels.map(([x, y]) => {
    const p = RT.pick(w, h, scene, x, y);
    if (p === null) return null;
    p.objectIsScene = p.object === scene.objects[p.index];
    delete p.object;
    return p;
  });
  const server = S.createServer();
  await new Promise((res) => server.listen(0, '127.0.0.1', res));
  const port = server.address().port;
  out.http = [];
  for (const [x, y] of out.pixels) {
    const g = await get(port, '/pick?scene=default14&w=' + w + '&h=' + h + '&x=' + x + '&y=' + y);
    out.http.push(g.status === 200 ? JSON.parse(g.body) : {status: g.status, body: g.body});
  }
  let name = 'picked';
  try { RT.pick(w, h, scene, w, 0); } catch (e) { name = e.name; }
  out.outside = {pick: name, status: (await get(port, '/pick?scene=default14&w=' + w + '&h=' + h + '&x=3&y=' + h)).status};
  server.close();
  RT.shutdown();
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
