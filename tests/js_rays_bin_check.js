'use strict';
// Driven by tests/test_gpu_rays_order.py: RT.traceRays with {bin: true} against the same call without it.
//   node js_rays_bin_check.js <package dir> <scene name> <base64 rays>
const [pkg, name, b64] = process.argv.slice(2);
const fs = require('fs'), path = require('path');
const RT = require(path.join(pkg, 'js', 'index.js')), F = require(path.join(pkg, 'js', 'flatten.js'));
const scene = F.sceneFromJSON(fs.readFileSync(path.join(pkg, 'scenes', name + '.json'), 'utf8'), path.join(pkg, 'scenes'));
const bytes = Buffer.from(b64, 'base64');
const rays = new Float64Array(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength));
const want = {rgb: true, rgba: true, hits: true};
const plain = RT.traceRays(scene, rays, want), binned = RT.traceRays(scene, rays, Object.assign({bin: true}, want));
const raw = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const hit = (h) => h && [h.index, h.inside, h.t, h.point, h.normal, h.u, h.v];
const same = raw(plain.rgb).equals(raw(binned.rgb)) && raw(plain.rgba).equals(raw(binned.rgba)) &&
  JSON.stringify(plain.hits.map(hit)) === JSON.stringify(binned.hits.map(hit));
RT.shutdown();
console.log(JSON.stringify({same, rgba: Array.from(binned.rgba)}));
