'use strict';
// Driven by tests/test_gpu_rays.py: RT.traceRays and GET /ray for rays handed over as base64 binary64 bytes.
//   node js_rays_check.js <package dir> <scene name> <base64 rays>
const [pkg, name, b64] = process.argv.slice(2);
const fs = require('fs'), http = require('http'), path = require('path');
const RT = require(path.join(pkg, 'js', 'index.js')), F = require(path.join(pkg, 'js', 'flatten.js')), S = require(path.join(pkg, 'js', 'server.js'));
const scene = F.sceneFromJSON(fs.readFileSync(path.join(pkg, 'scenes', name + '.json'), 'utf8'), path.join(pkg, 'scenes'));
const bytes = Buffer.from(b64, 'base64');
const rays = new Float64Array(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength));
const r = RT.traceRays(scene, rays, {rgb: true, rgba: true, hits: true});
const out = {
  rgb: Buffer.from(r.rgb.buffer, r.rgb.byteOffset, r.rgb.byteLength).toString('base64'),
  rgba: Array.from(r.rgba),
  hits: r.hits.map((h) => h && {index: h.index, inside: h.inside, t: h.t, point: h.point, normal: h.normal, u: h.u, v: h.v}),
};
const server = S.createServer();
server.listen(0, '127.0.0.1', () => {
  const port = server.address().port;
  const get = (p) => new Promise((res) => http.get({host: '127.0.0.1', port, path: p}, (m) => {
    let body = ''; m.on('data', (d) => { body += d; }); m.on('end', () => res({status: m.statusCode, body: JSON.parse(body)}));
  }));
  const q = ['ox', 'oy', 'oz', 'dx', 'dy', 'dz'].map((k, i) => k + '=' + encodeURIComponent(String(rays[i]))).join('&');
  Promise.all([get('/ray?scene=' + name + '&' + q), get('/ray?scene=' + name + '&ox=1'), get('/ray?scene=' + name + '&' + q + '&segs=17'), get('/ray?scene=nope&' + q)])
    .then(([ok, a, b, c]) => { out.bridge = ok; out.bad = [a.status, b.status, c.status]; server.close(); RT.shutdown(); console.log(JSON.stringify(out)); });
});
