/* etgsim_render.h -- camera images of the simulated robots: the getCameraImage of the reference's evaluation loops.
 *
 * train.py:196-199 (and BCtrain.py:163-165) grab a 640 x 480 frame with p.getCameraImage after every evaluation step.  Each image
 * here shows ONE robot on ITS OWN terrain (robots never interact; robot e walks on heightfield band e % hf_bands): the trunk
 * collision box, per leg a hip sphere, thigh and calf capsules and the foot sphere, placed by the physics tick's own leg
 * kinematics, over the plane z = 0 or the robot's heightfield band, lit by one directional light with shadows cast by the robot.
 * The same library as etgsim.h (its ABI version, 2, is unchanged); this header declares the one entry point that is not part of
 * etgsim.h.
 *
 * Contract of etg_render:
 *   h                 the simulator: its terrain and robot geometry.  Rendering reads only its arguments and these constants; it
 *                     changes no simulator state.
 *   state [n,37]      the state rows to draw (etg_get_state layout: pos3, quat4 xyzw, ..., q12 at column 13).
 *   env_ids [n]       the env id of each image, in [0, N): its terrain band is id % hf_bands.
 *   view, proj [n,16] per image, column-major 4 x 4 matrices as pybullet's computeViewMatrix (gluLookAt) and
 *                     computeProjectionMatrixFOV (gluPerspective) produce them.
 *   width, height     1 .. 4096.  Image row 0 is the top row; one ray through each pixel centre.
 *   rgba [n,H,W,4]    required, uint8, 4-byte aligned: r, g, b, 255.
 *   depth [n,H,W]     optional (NULL): float32, the OpenGL depth-buffer value 0.5 z_ndc + 0.5 (pybullet's depth image), 1 for sky.
 *   seg [n,H,W]       optional (NULL): int32, -1 sky, 0 terrain, 1 trunk, 2 + 4 leg + {0 hip, 1 thigh, 2 calf, 3 foot}.
 * A null handle, a null required pointer, n <= 0, a size outside 1..4096 or an env id outside [0, N) returns ETG_ERR_BAD_ARG.
 * The call waits for `stream` once (it checks the env ids on the host).  Pointers are device pointers.                       */
#ifndef ETGSIM_RENDER_H_
#define ETGSIM_RENDER_H_

#include "etgsim.h"

#ifdef __cplusplus
extern "C" {
#endif

int etg_render(EtgHandle* h, const float* state, const int* env_ids, int n, const float* view, const float* proj, int width,
               int height, uint8_t* rgba, float* depth, int* seg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETGSIM_RENDER_H_ */
