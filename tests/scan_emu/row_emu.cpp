// TEST-ONLY host build of scan_core.h's row_of_base (the row the closed-loop kernels with SCAN make from the seven base values
// they hold in registers) next to the path etg_height_scan takes for the same robot: state_pose on the base columns, then
// make_row.  Both write c, s and the position of each row; the test compares their bits.
#include <stdint.h>

#include "../../paddlerobotics_amd/csrc/scan_core.h"

using namespace etg;
using namespace etg::scan;

static void put(const Row& r, float* out) {
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.c; out[4] = r.s; out[5] = (float)r.env;
}

// base7 [n,7]: x, y, z, qx, qy, qz, qw per robot -> by_values [n,6], by_columns [n,6]: x, y, z, cos, sin, env
extern "C" void remu_rows(const float* base7, int n, float* by_values, float* by_columns) {
  float* base = new float[(size_t)BS_N * n]();
  const int col[7] = {BS_PX, BS_PY, BS_PZ, BS_QX, BS_QY, BS_QZ, BS_QW};
  for (int e = 0; e < n; e++)
    for (int k = 0; k < 7; k++) base[(size_t)col[k] * n + e] = base7[(size_t)e * 7 + k];
  for (int e = 0; e < n; e++) {
    const float* v = base7 + (size_t)e * 7;
    put(row_of_base(v[0], v[1], v[2], v[3], v[4], v[5], v[6], e), by_values + (size_t)e * 6);
    float pose[4];
    state_pose(base, n, e, pose);
    put(make_row(pose, e), by_columns + (size_t)e * 6);
  }
  delete[] base;
}
