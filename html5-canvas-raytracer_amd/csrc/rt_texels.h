// Launch record of the texel blit (rt_texels.hip), shared with its host side (rt_scene.hip: rt_scene_set_texels*).  Not part of the ABI.
#ifndef RT_TEXELS_H
#define RT_TEXELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define RT_TEXELS_WG 256u

// Passed by value in the kernarg segment: everything here is wave-uniform.  Pitches are in texels (dwords): row j of the rectangle is
// src + j * src_pitch -> dst + j * dst_pitch, w texels.
struct rt_texels_launch {
  uint32_t *dst;                   // the rectangle's first texel inside the resident blob (4-byte aligned: rt_scene_validate)
  const uint32_t *src;             // device memory, or pinned host memory the device reads (the host form's staged rows)
  uint64_t dst_pitch, src_pitch;
  uint32_t w;
};

// h <= 16384 rows (a texture's height: rt_scene_validate), w >= 1.  Returns a hipError_t as int.
extern "C" int rt_launch_texels_blit(const rt_texels_launch *L, uint32_t h, hipStream_t stream);

#endif
