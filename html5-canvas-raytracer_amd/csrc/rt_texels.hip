// rt_texels.hip — the texel blit of rt_scene_set_texels / rt_scene_set_texels_device (include/rt_hip.h): h source rows of w RGBA8 texels
// into a rectangle of a resident texture.  One dword per work-item, grid (ceil(w / 256), h): the row is the workgroup's y, the column
// its x * 256 + the lane - no division, no loop.  A texel is one aligned dword on both sides (the source is only known to be 4-byte
// aligned), so a wave's 64 loads and 64 stores are 256 contiguous bytes each.  Ordered against the scene's launches by stream and
// event alone (rt_scene.hip): nothing here is read or written by another kernel while this one runs.  No test switches: one object
// for both libraries.
#include "rt_texels.h"

__global__ void __launch_bounds__(RT_TEXELS_WG) rt_texels_blit(const rt_texels_launch L) {
  const uint32_t x = blockIdx.x * RT_TEXELS_WG + threadIdx.x;
  if (x >= L.w) return;
  const uint64_t y = blockIdx.y;
  L.dst[y * L.dst_pitch + x] = L.src[y * L.src_pitch + x];
}

extern "C" int rt_launch_texels_blit(const rt_texels_launch *L, uint32_t h, hipStream_t stream) {
  hipLaunchKernelGGL(rt_texels_blit, dim3((L->w + RT_TEXELS_WG - 1u) / RT_TEXELS_WG, h), dim3(RT_TEXELS_WG), 0, stream, *L);
  return (int)hipGetLastError();
}
