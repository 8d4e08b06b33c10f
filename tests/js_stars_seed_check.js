'use strict';
// Driven by tests/test_gpu_stars_seed.py: the Node host animates the stars sampler's seed the way the README shows
// (scene.starsSeed = frame; RT.render(..., {into: data})) and asks the HTTP bridge for a seeded frame.
//   node tests/js_stars_seed_check.js OUT_DIR W H
// writes OUT_DIR/seed<N>.rgba for the RT.render frames and OUT_DIR/http9.rgba for /frame?...&seed=9; prints a JSON line.
const http = require('http');
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..');
const RT = require(path.join(ROOT, 'html5-canvas-raytracer_amd', 'js', 'index.js'));
const F = require(path.join(ROOT, 'html5-canvas-raytracer_amd', 'js', 'flatten.js'));
const S = require(path.join(ROOT, 'html5-canvas-raytracer_amd', 'js', 'server.js'));

const [outDir, W, H] = [process.argv[2], parseInt(process.argv[3], 10), parseInt(process.argv[4], 10)];
const SC = path.join(ROOT, 'html5-canvas-raytracer_amd', 'scenes');
const get = (port, p) => new Promise((resolve, reject) => {
  http.get({host: '127.0.0.1', port, path: p}, (res) => { const c = []; res.on('data', (x) => c.push(x)); res.on('end', () => resolve({status: res.statusCode, body: Buffer.concat(c)})); }).on('error', reject);
});

(async () => {
  const scene = F.sceneFromJSON(fs.readFileSync(path.join(SC, 'default14_stars.json'), 'utf8'), SC);
  const out = {frames: []};
  let data = null;
  for (const seed of [0, 9]) {
    scene.starsSeed = seed;                                   // what the reference's Math.random() per redraw becomes
    const got = RT.render(W, H, scene, data ? {into: data} : undefined);
    if (data) out.reused = got === data;                      // the frame of the first render, filled again
    data = got;
    fs.writeFileSync(path.join(outDir, 'seed' + seed + '.rgba'), Buffer.from(data.buffer, data.byteOffset, data.length));
    out.frames.push(seed);
  }
  // the bridge: the seed is per request, the cached scene keeps seed 0
  const server = S.createServer();
  await new Promise((r) => server.listen(0, '127.0.0.1', r));
  const port = server.address().port;
  const a = await get(port, '/frame?scene=default14_stars&w=' + W + '&h=' + H + '&seed=9');
  const b = await get(port, '/frame?scene=default14_stars&w=' + W + '&h=' + H);
  server.close();
  out.http = [a.status, b.status];
  fs.writeFileSync(path.join(outDir, 'http9.rgba'), a.body);
  fs.writeFileSync(path.join(outDir, 'http.rgba'), b.body);
  RT.shutdown();
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
