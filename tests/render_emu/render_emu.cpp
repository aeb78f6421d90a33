// TEST-ONLY host build of the renderer source (paddlerobotics_amd/csrc/render_core.h): the per-pixel work of k_render
// (etg_render.hip) run by a plain loop, with the scene packed from the same EtgConfig / EtgRobotModel the library receives.
#include <stdint.h>

#include "../../paddlerobotics_amd/csrc/render_core.h"

using namespace etg;
using namespace etg::render;

static RenderScene scene(const EtgConfig* cfg, const EtgRobotModel* model, const float* hf) {
  const KCfg K = make_kcfg(*cfg, *model);
  const ModelF M = make_modelf(*model);
  float lo = 0.0f, hi = 0.0f;
  if (cfg->terrain == 1 && hf) height_range(hf, (size_t)K.hf_nx * K.hf_ny * K.hf_bands, lo, hi);
  return make_render_scene(K, M, cfg->terrain == 1 ? hf : nullptr, lo, hi);
}

// etg_render on host pointers (no argument checks: the tests pass valid ones)
extern "C" void remu_render(const EtgConfig* cfg, const EtgRobotModel* model, const float* hf, const float* state,
                            const int* env_ids, int n, const float* view, const float* proj, int W, int H, uint8_t* rgba,
                            float* depth, int* seg) {
  const RenderScene S = scene(cfg, model, hf);
  for (int i = 0; i < n; i++) {
    Prims P;
    Camera cam;
    build_prims(S, state + (size_t)i * ETG_STATE_DIM, P);
    make_camera(view + (size_t)i * 16, proj + (size_t)i * 16, cam);
    const int band = S.terrain ? band_of(S, env_ids[i]) : 0;
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const size_t pix = ((size_t)i * H + y) * W + x;
        uint32_t c;
        float z;
        int s;
        shade_pixel(S, P, cam, band, x, y, W, H, c, z, s);
        for (int k = 0; k < 4; k++) rgba[4 * pix + k] = (uint8_t)(c >> (8 * k));
        depth[pix] = z;
        seg[pix] = s;
      }
  }
}

// the primitives' frame points of one state row: out[leg][o1, o2, o3, pf][3], world frame
extern "C" void remu_prims(const EtgConfig* cfg, const EtgRobotModel* model, const float* state, float* out) {
  const RenderScene S = scene(cfg, model, nullptr);
  Prims P;
  build_prims(S, state, P);
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) {
      out[(4 * l + 0) * 3 + k] = P.o1[l][k];
      out[(4 * l + 1) * 3 + k] = P.o2[l][k];
      out[(4 * l + 2) * 3 + k] = P.o3[l][k];
      out[(4 * l + 3) * 3 + k] = P.pf[l][k];
    }
}
