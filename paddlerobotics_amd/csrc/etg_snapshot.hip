// etg_snapshot.hip -- gfx950 kernel of etg_snapshot_save / etg_snapshot_restore (include/etgsim_snapshot.h): a plain gather /
// scatter between the field-major state arrays and robot-major records.
//
// Mapping: one lane per word of a record; a workgroup of 256 lanes covers 256 consecutive words of ONE record, so the record
// side is read / written in full lines and the array side in strides of the robot count.  Not time-critical (a save or restore
// happens once per many thousand steps), so nothing is staged.
#include "snapshot_core.h"

namespace etg {
namespace snapshot {

__global__ void __launch_bounds__(256) k_snapshot(Table T, const int32_t* ids, int n, uint32_t* rows, int blocks_per_row, int write) {
  const int rec = blockIdx.x / blocks_per_row;
  const int w = (blockIdx.x - rec * blocks_per_row) * 256 + threadIdx.x;
  if (rec >= n || w >= T.row_words) return;
  const int env = ids ? ids[rec] : rec;
  if (env < 0 || env >= T.n_env) return;   // (checked on the host already: never an access outside the arrays)
  uint32_t* cell = rows + (size_t)rec * T.row_words + w;
  if (w < kHeadWords) {
    if (!write) *cell = w == 0 ? (uint32_t)env : 0u;
    return;
  }
  const size_t N = (size_t)T.n_env;
  for (int s = 0; s < T.nseg; s++) {
    const Seg& g = T.seg[s];
    const int k = w - g.off;
    if (k < 0 || k >= g.rows * g.per) continue;
    if (!g.p) {                      // not allocated: zeros out, nothing in
      if (!write) *cell = 0u;
      return;
    }
    if (g.bytes) {
      unsigned char* b = (unsigned char*)g.p + env;
      if (write) *b = (unsigned char)(*cell != 0u);
      else *cell = (uint32_t)*b;
      return;
    }
    const int r = k / g.per, c = k - r * g.per;
    uint32_t* a = (uint32_t*)g.p + (size_t)r * g.per * N + (size_t)g.per * env + c;
    if (write) *a = *cell;
    else *cell = *a;
    return;
  }
  if (!write) *cell = 0u;            // the padding behind the last segment
}

}  // namespace snapshot
}  // namespace etg

hipError_t etg_snapshot_launch(const etg::snapshot::Table& T, const int32_t* ids, int n, uint32_t* rows, int write, hipStream_t stream) {
  const int bpr = (T.row_words + 255) / 256;
  hipLaunchKernelGGL(etg::snapshot::k_snapshot, dim3((unsigned)bpr * (unsigned)n), dim3(256), 0, stream, T, ids, n, rows, bpr, write);
  return hipGetLastError();
}
