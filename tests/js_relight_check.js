// js_relight_check - relit nodes from Node for tests/test_node_relight.py:
//   node js_relight_check.js <package dir> <w> <h>     default14's primary rays at w x h: RT.relightRays (a walked table, pix, base; the
//                                                      defaults), RT.traceRays(..., {soft}) (one level, every level, the defaults), the plain
//                                                      wavefront trace beside them, and what a malformed `soft` throws
// prints one line of JSON; binary data is base64.
const pkg = process.argv[2], w = Number(process.argv[3]), h = Number(process.argv[4]);
const RT = require(pkg + '/js/index.js'), F = require(pkg + '/js/flatten.js'), fs = require('fs');
const b64 = (a) => (a ? Buffer.from(a.buffer || a, a.byteOffset || 0, a.byteLength).toString('base64') : null);
const sc = F.sceneFromJSON(fs.readFileSync(pkg + '/scenes/default14.json', 'utf8'), pkg + '/scenes');
const rays = RT.primaryRays(w, h, sc), n = rays.length / 6;
const offsets = RT.lightingOffsets(8);
const pix = Uint32Array.from({length: n}, (_, i) => n - 1 - i);
const walked = RT.relightRays(sc, rays, {samples: 5, lightRadius: 1, offsets, stride: 7, base: 11, pix});
const plain = RT.relightRays(sc, rays, {samples: 4, lightRadius: 0.5});
const shaded = RT.shadeRays(sc, rays);
const node = walked.node(n >> 1);
const want = {rgb: true, rgba: true};
const one = RT.traceRays(sc, rays, Object.assign({soft: {samples: 4, lightRadius: 1, offsets, stride: 1}}, want));
const all = RT.traceRays(sc, rays, Object.assign({soft: {samples: 4, lightRadius: 1, offsets, stride: 1, levels: sc.segs, base: 3}}, want));
const dflt = RT.traceRays(sc, rays, Object.assign({soft: {samples: 3, lightRadius: 0.5}}, want));
const hard = RT.traceRays(sc, rays, Object.assign({wavefront: true}, want));
const refused = [];
for (const soft of [null, 7, {}, {samples: 0, lightRadius: 1}, {samples: 2}, {samples: 2, lightRadius: '1'}, {samples: 2, lightRadius: 1, offsets: [0, 0, 1]},
  {samples: 2, lightRadius: 1, offsets: new Float64Array(4)}, {samples: 2, lightRadius: 1, levels: -1}, {samples: 2, lightRadius: 1, stride: 0.5}]) {
  try { RT.traceRays(sc, rays, {soft}); refused.push('accepted'); } catch (e) { refused.push(e.constructor.name); }
}
try { RT.traceRays(sc, rays, {soft: {samples: 2, lightRadius: 1}, hits: true}); refused.push('accepted'); } catch (e) { refused.push(e.constructor.name); }
try { RT.relightRays(sc, rays, {lightRadius: 1}); refused.push('accepted'); } catch (e) { refused.push(e.constructor.name); }
const pic = (r) => ({rgb: b64(r.rgb), rgba: b64(r.rgba), levelCounts: r.levelCounts, type: Object.prototype.toString.call(r.rgba)});
console.log(JSON.stringify({rays: b64(rays), walked: b64(new Uint8Array(walked.nodes)), count: walked.count, plain: b64(new Uint8Array(plain.nodes)),
  shaded: b64(new Uint8Array(shaded.nodes)), node: {diffuse: node.diffuse, specular: node.specular, index: node.hit ? node.hit.index : -1},
  one: pic(one), all: pic(all), dflt: pic(dflt), hard: pic(hard), refused}));
