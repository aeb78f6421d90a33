// etg_render.hip -- gfx950 kernel of etg_render (include/etgsim_render.h): camera images, one robot on its own terrain each.
//
// Mapping: a workgroup of 256 lanes covers a 16 x 16 pixel tile of one image, each wave64 an 8 x 8 block of it, so the rays of a
// wave stay coherent (they mostly take the same bounding-sphere, primitive and march branches).  Lane 0 builds the image's 17
// primitives and camera inverse once into LDS; every lane then reads them from there (same address across the wave: broadcast)
// and shades its pixel (render_core.h: shade_pixel), written as one 32-bit rgba store per lane.
#include <hip/hip_runtime.h>

#include "render_core.h"

namespace etg {
namespace render {

constexpr int kTile = 16;   // pixels per side of a workgroup's tile: 2 x 2 waves of 8 x 8

__global__ void __launch_bounds__(256) k_render(RenderScene S, const float* state, const int* env_ids, const float* view,
                                                const float* proj, int W, int H, int tiles_x, int tiles, uint32_t* rgba,
                                                float* depth, int* seg) {
  __shared__ Prims P;
  __shared__ Camera cam;
  __shared__ int band;
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  if (threadIdx.x == 0) {
    build_prims(S, state + (size_t)img * ETG_STATE_DIM, P);
    make_camera(view + (size_t)img * 16, proj + (size_t)img * 16, cam);
    band = S.terrain ? band_of(S, env_ids[img]) : 0;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = (tile % tiles_x) * kTile + (wave & 1) * 8 + (lane & 7);
  const int y = (tile / tiles_x) * kTile + (wave >> 1) * 8 + (lane >> 3);
  if (x >= W || y >= H) return;
  uint32_t c;
  float z;
  int s;
  shade_pixel(S, P, cam, band, x, y, W, H, c, z, s);
  const size_t pix = ((size_t)img * H + y) * W + x;
  rgba[pix] = c;
  if (depth) depth[pix] = z;
  if (seg) seg[pix] = s;
}

}  // namespace render
}  // namespace etg

hipError_t etg_render_launch(const etg::render::RenderScene& S, const float* state, const int* env_ids, int n, const float* view,
                             const float* proj, int width, int height, uint8_t* rgba, float* depth, int* seg, hipStream_t stream) {
  using etg::render::kTile;
  const int tx = (width + kTile - 1) / kTile, ty = (height + kTile - 1) / kTile;
  hipLaunchKernelGGL(etg::render::k_render, dim3((unsigned)(tx * ty) * (unsigned)n), dim3(256), 0, stream, S, state, env_ids, view,
                     proj, width, height, tx, tx * ty, (uint32_t*)rgba, depth, seg);
  return hipGetLastError();
}
