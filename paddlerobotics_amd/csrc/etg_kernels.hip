// etg_kernels.hip -- gfx950 kernels + C-ABI of the batched A1 simulator (include/etgsim.h).
//
// Two lane mappings of the same algorithm over one HBM state layout (etg_layout.h):
//   k_step16 / k_settle16 / k_finish16 (etg_core16.h): one robot = one 16-lane DPP row, a wave64 = 4 robots;
//       4096 robots = 1024 single-wave workgroups = one wave on every SIMD (the default up to 4096 robots);
//   k_step / k_settle / k_finish (etg_core.h): one robot = one quad (one leg per lane), a wave64 = 16 robots
//       (bigger batches).
// Workgroups are remapped so that each XCD owns a contiguous range of robots (xcd_contiguous_block).  Reductions
// and broadcasts are DPP moves (quad_perm, row butterflies, row_newbcast), fused into the consuming ALU op where
// possible (v_add_f32_dpp by the compiler, v_fmac_f32_dpp by inline asm); the 4-lane contact operator's 4x4
// blocks are v_mfma_f32_4x4x1.  LDS holds each lane's private per-step parameter column (no barriers anywhere);
// the per-tick constants go straight from HBM to registers.  A reset restores the cached 500-tick settle.
// Every step / rollout / reset kernel has compile-time variants: flat ground vs heightfield, body contacts, and PLAIN (the
// default robot layer with its unused options compiled out).  etg_layout.h lists them and picks one per launch (dispatch16 /
// dispatch4, which LAUNCH16 / LAUNCH4 and the test emulation call).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "etg_core16.h"
#include "gram16.h"
#include "policy_core.h"
#include "scan_core.h"
#include "../../include/etgsim_step_policy.h"
#include "../../include/etgsim_scan_policy.h"
#include "../../include/etgsim_collect.h"
#include "../../include/etgsim_monitor.h"
#include "../../include/etgsim_terminal.h"

// ---- translation units.  The device code of this file is ~120 instantiations of the physics tick: four minutes of
// single-threaded code generation.  paddlerobotics_amd/build.py therefore compiles the file ETG_TU_PARTS times in parallel:
// part 0 holds the host side (the C-ABI) and the small kernels and declares the tick kernels `extern template`; parts 1..
// hold their explicit instantiations (the table at the end of namespace etg).  Without the macros -- tools/build_variant.sh, a
// plain `hipcc etg_kernels.hip` -- the file is one unit and every kernel is instantiated where it is launched, as before.
#ifndef ETG_TU_PARTS
#define ETG_TU_PARTS 1
#define ETG_TU_PART 0
#endif
#define ETG_TU_HOST (ETG_TU_PART == 0)

namespace etg {

// ---- DPP quad helpers -------------------------------------------------------------
// bound_ctrl = true: every lane of every group is always valid here, and with it the compiler needs no
// "old" value -- without it each v_mov_b32_dpp is preceded by a v_mov_b32 that zero-initialises the
// destination (measured: ~150 extra VALU issues per tick)
template <int CTRL> __device__ __forceinline__ float dpp_(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

struct GpuCtx {
  int gid, env, lane, N, NL;
  const float* lds;  // this lane's parameter column in LDS: lds[k * BLOCK]
  const float* gpar; // D.par, for the tick constants read straight into registers
  // store gate (fused rollouts under KCfg.stop_at_done, etg_core16.h: control_step16_core): every store of this context happens
  // on the lanes inside the gate only.  Never closed by the step / reset kernels: the constant `true` folds away there.
  mutable bool gate = true;
  __device__ __forceinline__ void set_gate(bool on) const { gate = on; }
  __device__ __forceinline__ void open_gate() const { gate = true; }
  __device__ __forceinline__ int sel_i(bool m, int a, int b) const { return m ? a : b; }
  __device__ __forceinline__ float par(int k) const { return lds[k * 64]; }
  __device__ __forceinline__ float tpar(int k) const { return gpar[(size_t)k * NL + gid]; }
  __device__ __forceinline__ float ld_lane(const float* p, int f) const { return p[(size_t)f * NL + gid]; }
  __device__ __forceinline__ void st_lane(float* p, int f, float v) const { if (gate) p[(size_t)f * NL + gid] = v; }
  __device__ __forceinline__ float ld_env(const float* p, int f) const { return p[(size_t)f * N + env]; }
  __device__ __forceinline__ void st_env(float* p, int f, float v) const { if (gate && lane == 0) p[(size_t)f * N + env] = v; }
  __device__ __forceinline__ int ld_env_i(const int* p, int f) const { return p[(size_t)f * N + env]; }
  __device__ __forceinline__ void st_env_i(int* p, int f, int v) const { if (gate && lane == 0) p[(size_t)f * N + env] = v; }
  __device__ __forceinline__ void st_ring(float* r, int slot, int k, float v) const { if (gate) r[((size_t)slot * 8 + k) * NL + gid] = v; }
  __device__ __forceinline__ float ld_ring(const float* r, int slot, int k) const { return r[((size_t)slot * 8 + k) * NL + gid]; }
  // the ring is written and read back by the SAME lane (program order): no fence needed
  __device__ __forceinline__ void ring_fence() const {}
  // phase boundary: keep the machine scheduler from interleaving whole phases of the tick
  // (it otherwise stretches live ranges to >500 registers and spills)
  __device__ __forceinline__ void phase([[maybe_unused]] int id) const {
    __builtin_amdgcn_sched_barrier(0);
#ifdef ETG_PROFILE_PHASES  // tools/phase_profile.py: per-phase s_memtime deltas of one wave
    long long t = clock64();
    prof[id] += t - prof_last;
    prof_last = t;
    __builtin_amdgcn_sched_barrier(0);
#endif
  }
#ifdef ETG_PROFILE_PHASES
  mutable long long prof[16];
  mutable long long prof_last;
#endif
  int row_base = 0;  // first robot of the [*, rowlen] row buffers (observation tile in LDS: the workgroup's first robot)
  __device__ __forceinline__ void st_row_env(float* p, int rowlen, int col, float v) const { if (gate && lane == 0) p[(size_t)(env - row_base) * rowlen + col] = v; }
  __device__ __forceinline__ void st_row_lane(float* p, int rowlen, int col0, int stride, float v) const { if (gate) p[(size_t)(env - row_base) * rowlen + col0 + stride * lane] = v; }
  __device__ __forceinline__ float ld_row_env(const float* p, int rowlen, int col) const { return p[(size_t)(env - row_base) * rowlen + col]; }
  __device__ __forceinline__ float ld_row_lane(const float* p, int rowlen, int col0, int stride) const { return p[(size_t)(env - row_base) * rowlen + col0 + stride * lane]; }
  // order-symmetric quad sum: (x0+x1)+(x2+x3) on every lane, bit-identical across the quad
  __device__ __forceinline__ float qsum(float a) const {
    float t = a + dpp_<0xB1>(a);  // quad_perm [1,0,3,2]
    return t + dpp_<0x4E>(t);     // quad_perm [2,3,0,1]
  }
  __device__ __forceinline__ float qmax(float a) const {
    float t = fmaxf(a, dpp_<0xB1>(a));
    return fmaxf(t, dpp_<0x4E>(t));
  }
  __device__ __forceinline__ float qbcast(float a, int j) const {  // j is a constant after unrolling
    switch (j) {
      case 0: return dpp_<0x00>(a);
      case 1: return dpp_<0x55>(a);
      case 2: return dpp_<0xAA>(a);
      default: return dpp_<0xFF>(a);
    }
  }
  // acc[i] += a@lane_i * b@this_lane for the 4 lanes of the quad: v_mfma_f32_4x4x1_16b_f32 computes
  // 16 independent 4x4 outer products per wave64, block b = lanes 4b..4b+3, D[i][j] = A[lane i] *
  // B[lane j] held at lane j / register i (layout verified on hardware: tools/ubench/mfma4x4.hip)
  __device__ __forceinline__ void quad_outer(float a, float b, float* acc) const {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 v = {acc[0], acc[1], acc[2], acc[3]};
    v = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, v, 0, 0, 0);
    acc[0] = v[0]; acc[1] = v[1]; acc[2] = v[2]; acc[3] = v[3];
  }
  __device__ __forceinline__ bool lane_is(int j) const { return lane == j; }
  __device__ __forceinline__ bool any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0ull; }
  __device__ __forceinline__ unsigned uniform_bits(unsigned v) const { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }   // a wave-uniform value, kept in an SGPR
  __device__ __forceinline__ bool wave_any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0ull; }   // "does any robot of the wave need another sweep?"
  // "does any lane of MY robot (quad) see b?" from the wave mask of the compare: two ANDs with this lane's quad field
  __device__ __forceinline__ bool robot_any(bool b) const {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(b);
    const unsigned sh = (unsigned)(threadIdx.x & 28);           // first lane of the quad inside its 32-lane half
    const unsigned f = 0xFu << sh;
    return ((threadIdx.x & 32) ? ((unsigned)(m >> 32) & f) : ((unsigned)m & f)) != 0u;
  }
  __device__ __forceinline__ int uniform_int(float a) const { return (int)a; }
  __device__ __forceinline__ void terrain(const KCfg& K, float x, float y, float& h, float& nx, float& ny, float& nz) const {
    if (K.terrain == 0) { h = 0.0f; nx = 0.0f; ny = 0.0f; nz = 1.0f; }
    else heightfield_query(K, env, x, y, h, nx, ny, nz);
  }
  __device__ __forceinline__ void terrain_fetch(const KCfg& K, float x, float y, float* tap) const { heightfield_fetch(K, env, x, y, tap); }
  __device__ __forceinline__ void terrain_finish(const KCfg& K, const float* tap, float& h, float& nx, float& ny, float& nz) const {
    heightfield_finish(K, tap, h, nx, ny, nz);
  }
};

// FLAT selects the plane-z=0 fast path at compile time (contact frame = rows of R, no terrain lookup)
// PLAIN: see GpuCtx16T.  BODY: body contact rows per leg compiled in (EtgConfig.body_contacts 1 / 2 -> 1, 3 -> 3)
template <bool FLAT, bool PLAIN = false, int BODY = 0> struct GpuCtxT : GpuCtx {
  static constexpr bool kFlat = FLAT; static constexpr bool kPlain = PLAIN; static constexpr int kBody = BODY;
};

// Workgroups are dealt round-robin to the 8 XCDs (block b -> XCD b % 8), each with its own L2.  Robots
// of neighbouring blocks share 128 B lines of the SoA state (a block covers only 16-64 B of a field), so
// give every XCD a CONTIGUOUS range of robots: the blocks that share a line then share an L2 and the
// line is fetched from HBM once instead of once per XCD.  Bijective for any grid size.
__device__ __forceinline__ int xcd_contiguous_block() {
  const int nb = gridDim.x, b = blockIdx.x, x = b & 7, q = nb >> 3, r = nb & 7;
  return x * q + (x < r ? x : r) + (b >> 3);
}

__device__ __forceinline__ bool make_ctx(const KCfg& K, GpuCtx& c) {
  c.gid = (K.block0 + xcd_contiguous_block()) * blockDim.x + threadIdx.x;   // (block0: etg_step_range; 0 in every other launch)
  c.N = K.n_env;
  c.NL = 4 * K.n_env;
  c.env = c.gid >> 2;
  c.lane = c.gid & 3;
  c.lds = nullptr;
  return c.gid < c.NL;
}

constexpr int BLOCK = 64;

// Parameters waiting for a robot's NEXT episode (etg_prepare_next_dynamics): the derived per-leg rows, the dynamic_param row and a
// pending flag per robot.  The settle that belongs to them already sits in the robot's settle cache; the restart inside
// etg_step_autoreset (or the next etg_reset of the robot) installs the rows.  All null when the feature is unused.
struct NextDyn { float* par; float* dyn; unsigned char* ok; };
// What an in-launch restart overwrites, kept by the AR step kernels for etg_step_autoreset_terminal (include/etgsim_terminal.h):
// the step's observation row of every robot (written from the values that produce it: next to the row of `obs` on 16 lanes,
// instead of it on 4 -- step4_body), and for each
// restarted robot the pre-restart values its extra sensor columns read (term_ctx_store).  Both null from etg_step_autoreset.
struct TermOut { float* obs; float* ctx; };
// the terminal_ctx row of a robot whose restart follows (lane `lane` of the robot's `lanes`): the episode step index of its
// terminal row (IC_STEP after the step), the step's trunk force (set + push: the restart clears the push) and its dynamic_param
// row (a restart on prepared next-episode rows replaces it).  Called before the restart touches any of them.
__device__ __forceinline__ void term_ctx_store(const KCfg& K, const DevState& D, int env, int lane, int lanes, int step, float* ctx) {
  const int N = K.n_env;
  float* row = ctx + (size_t)env * ETG_TERM_CTX_DIM;
  if (lane == 0) row[ETG_TERM_STEP] = (float)step;
  if (lane < 3) row[ETG_TERM_FORCE + lane] = D.ctl[(size_t)(CT_FEXT + lane) * N + env] + D.ctl[(size_t)(CT_PUSH + lane) * N + env];
  for (int k = lane; k < ETG_DYN_DIM; k += lanes) row[ETG_TERM_DYN + k] = D.dyn[(size_t)env * ETG_DYN_DIM + k];
}
// install the pending rows of the masked robots (a reset of theirs is about to use the settle cache that belongs to the rows)
#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void __launch_bounds__(256) k_next_take(KCfg K, DevState D, NextDyn NX, const uint8_t* mask) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = K.n_env, NL = 4 * N;
  if (col >= NL) return;
  const int env = col >> 2;
  if ((mask && !mask[env]) || !NX.ok[env]) return;
  for (int k = 0; k < PR_DERIVED; k++) D.par[(size_t)k * NL + col] = NX.par[(size_t)k * NL + col];
  for (int k = col & 3; k < ETG_DYN_DIM; k += 4) D.dyn[(size_t)env * ETG_DYN_DIM + k] = NX.dyn[(size_t)env * ETG_DYN_DIM + k];
}
// etg_prepare_next_dynamics replaces a robot's settle cache -- cached state AND the cache's copy of the latency ring -- while the
// robot keeps running.  A running robot still READS that ring copy for every delayed reading of a tick at or before its reset
// tick (ring_of_tick / KCfg.cring), i.e. during the first RING ticks of its episode.  Such YOUNG robots are left out of the
// call: out[env] = masked && the robot's episode is at least RING ticks old.  Their pending flag stays 0, so the caller's next
// refresh draws rows for them again.
__global__ void __launch_bounds__(256) k_next_old_enough(KCfg K, DevState D, const uint8_t* mask, uint8_t* out) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= K.n_env) return;
  out[env] = ((!mask || mask[env]) && D.ictl[(size_t)IC_TICK * K.n_env + env] - K.settle_ticks >= RING) ? 1 : 0;
}
// ok[env] = value for the masked robots; scratch flags start as "not cached" so that the settle runs for them
__global__ void __launch_bounds__(256) k_next_flags(KCfg K, unsigned char* ok, const uint8_t* mask, unsigned char value) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= K.n_env || (mask && !mask[env])) return;
  ok[env] = value;
}
#endif


// Stage the lane's 66 derived parameters in LDS, [field][lane] (conflict-free: lane i hits
// bank i).  Each lane reads back only its own column, so no barrier is needed -- the LDS
// is a software-managed register file extension here, not a sharing medium.
// only what the once-per-step code reads through c.par(); the tick constants go straight to registers (tpar)
constexpr int kStaged4[] = {PR_O1, PR_O1 + 1, PR_O1 + 2, PR_SY, PR_LAT_N, PR_LAT_A, PR_BASE_FOOT, PR_BASE_FOOT + 1,
                            PR_BASE_FOOT + 2, PR_POSE, PR_POSE + 1, PR_POSE + 2, PR_EMEAN, PR_EMEAN + 1, PR_EMEAN + 2,
                            PR_ESTD, PR_ESTD + 1, PR_ESTD + 2, PR_HIPSIGN};
constexpr int kNStaged4 = sizeof(kStaged4) / sizeof(int);
// issue / commit: a caller may put its own cold loads between the two (step4_body, like step16_body)
__device__ __forceinline__ void stage4_issue(GpuCtx& c, const DevState& D, float* lds_par, float (&v)[kNStaged4]) {
#pragma unroll
  for (int i = 0; i < kNStaged4; i++) v[i] = D.par[(size_t)kStaged4[i] * c.NL + c.gid];
  c.lds = lds_par + threadIdx.x;
  c.gpar = D.par;
}
__device__ __forceinline__ void stage4_commit(const GpuCtx& c, const float (&v)[kNStaged4]) {
  float* mine = const_cast<float*>(c.lds);
#pragma unroll
  for (int i = 0; i < kNStaged4; i++) mine[kStaged4[i] * BLOCK] = v[i];
}
__device__ __forceinline__ void stage_params(GpuCtx& c, const DevState& D, float* lds_par) {
  float v[kNStaged4];
  stage4_issue(c, D, lds_par, v);
  stage4_commit(c, v);
}

// the same staging for a wave of a multi-wave workgroup (its own [PR_N][64] area, lane = lane in the wave)
__device__ __forceinline__ void stage_params_wave(GpuCtx& c, const DevState& D, float* lds_wave, int lane) {
  constexpr int kStaged[] = {PR_O1, PR_O1 + 1, PR_O1 + 2, PR_SY, PR_LAT_N, PR_LAT_A, PR_BASE_FOOT, PR_BASE_FOOT + 1,
                             PR_BASE_FOOT + 2, PR_POSE, PR_POSE + 1, PR_POSE + 2, PR_EMEAN, PR_EMEAN + 1, PR_EMEAN + 2,
                             PR_ESTD, PR_ESTD + 1, PR_ESTD + 2, PR_HIPSIGN};
#pragma unroll
  for (int k : kStaged) lds_wave[k * 64 + lane] = D.par[(size_t)k * c.NL + c.gid];
  c.lds = lds_wave + lane;
  c.gpar = D.par;
}

#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void __launch_bounds__(BLOCK) k_set_params(KCfg K, ModelF M, DevState D, const float* dyn, const float* w,
                                                       const float* b, int per_env, const uint8_t* mask) {
  GpuCtx c;
  if (!make_ctx(K, c)) return;
  if (mask && !mask[c.env]) return;
  if (dyn) {
    if (c.lane == 0) D.cache_ok[c.env] = 0;   // the settle depends on the dynamic parameters
    float row[ETG_DYN_DIM], out[PR_DERIVED];
    for (int k = 0; k < ETG_DYN_DIM; k++) row[k] = dyn[(size_t)c.env * ETG_DYN_DIM + k];
    for (int k = c.lane; k < ETG_DYN_DIM; k += 4) D.dyn[(size_t)c.env * ETG_DYN_DIM + k] = row[k];   // kept for the dynamic_vec sensor
    derive_lane_params(M, row, c.lane, K.dt, out);
    for (int k = 0; k < PR_DERIVED; k++) D.par[(size_t)k * c.NL + c.gid] = out[k];   // (the strength ratios PR_STR.. are not derived: etg_set_motor_strength)
  }
  // the 63 ETG floats of a robot are copied by its 4 lanes (16 each)
  for (int k = c.lane; k < 60; k += 4)
    if (w) D.etgp[(size_t)(EP_W + k) * c.N + c.env] = w[(per_env ? (size_t)c.env * 60 : 0) + k];
  if (b && c.lane < 3) D.etgp[(size_t)(EP_B + c.lane) * c.N + c.env] = b[(per_env ? (size_t)c.env * 3 : 0) + c.lane];
}
#endif

// ---- reset = settle (only for robots without a valid settle cache) -> restore from the cache -> finish
// copy this lane's 8 ring words of all slots and its leg column between the live arrays and the cache
// (the ring is NOT copied back from the cache: readings of ticks up to the reset tick are served from KCfg.cring)
__device__ __forceinline__ void copy_leg_column(const DevState& D, size_t col, size_t NL, bool to_cache) {
  const float* src_leg = to_cache ? D.leg : D.cache_leg;
  float* dst_leg = to_cache ? D.cache_leg : D.leg;
  for (int f = 0; f < LG_N; f++) dst_leg[(size_t)f * NL + col] = src_leg[(size_t)f * NL + col];
}
__device__ __forceinline__ void copy_base_column(const DevState& D, int env, int N, bool to_cache) {
  const float* src = to_cache ? D.base : D.cache_base;
  float* dst = to_cache ? D.cache_base : D.base;
  for (int f = 0; f < BS_N; f++) dst[(size_t)f * N + env] = src[(size_t)f * N + env];
}

// A cached settle is reusable when it ran at the start offset the robot resets to now; on flat ground the settle is
// translation-invariant, so there any cached settle is reusable and k_cache_sync shifts it to the new offset.
template <bool FLAT> __device__ __forceinline__ bool settle_cached(const KCfg& K, const DevState& D, int env) {
  if (!D.cache_ok[env]) return false;
  if (FLAT) return true;
  return D.cache_off[env] == D.reset_off[env] && D.cache_off[K.n_env + env] == D.reset_off[K.n_env + env];
}
// every lane of the robot writes the same values (the robot's lanes share a wave: the reads above came first)
__device__ __forceinline__ void settle_mark_fresh(const KCfg& K, const DevState& D, int env, float ox, float oy) {
  D.cache_ok[env] = 0;   // "just settled": k_cache_sync snapshots the ring, k_cache_mark sets it again
  D.cache_off[env] = ox;
  D.cache_off[K.n_env + env] = oy;
}

template <bool FLAT, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(BLOCK) k_settle(KCfg K, DevState D, const uint8_t* mask) {
  GpuCtxT<FLAT, PLAIN, BODY> c;
  if (!make_ctx(K, c)) return;
  if ((mask && !mask[c.env]) || settle_cached<FLAT>(K, D, c.env)) return;   // whole quads drop out together
  __shared__ float lds_par[PR_N * BLOCK];
  stage_params(c, D, lds_par);
  LaneState<float> L;
  const float ox = D.reset_off[c.env], oy = D.reset_off[K.n_env + c.env];
  reset_settle(c, K, L, D.ring, ox, oy);
  store_state(c, D.cache_base, D.cache_leg, L);              // the ring is copied by k_cache_sync (needs the stores done)
  store_state(c, D.base, D.leg, L);
  settle_mark_fresh(K, D, c.env, ox, oy);
}

// one thread per leg column: after a settle, snapshot the ring into the cache and mark the robot cached;
// for every masked robot, bring state + ring back from the cache
#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void __launch_bounds__(256) k_cache_sync(KCfg K, DevState D, const uint8_t* mask) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = K.n_env, NL = 4 * N;
  if (col >= NL) return;
  const int env = col >> 2;
  if (mask && !mask[env]) return;
  if (!D.cache_ok[env]) {   // just settled by k_settle: live arrays -> cache (ring only; state was stored to both)
    for (int w = 0; w < RING * 8; w++) D.cache_ring[(size_t)w * NL + col] = D.ring[(size_t)w * NL + col];
  } else {                  // cached: cache -> live arrays
    copy_leg_column(D, col, NL, false);
    if ((col & 3) == 0) {
      copy_base_column(D, env, N, false);
      // shift to the offset of THIS reset (non-zero only on flat ground, see settle_cached)
      D.base[(size_t)BS_PX * N + env] += D.reset_off[env] - D.cache_off[env];
      D.base[(size_t)BS_PY * N + env] += D.reset_off[N + env] - D.cache_off[N + env];
    }
  }
}
__global__ void __launch_bounds__(256) k_cache_mark(KCfg K, DevState D, const uint8_t* mask) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= K.n_env) return;
  if (mask && !mask[env]) return;
  D.cache_ok[env] = 1;
}
#endif

template <bool FLAT, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(BLOCK) k_finish(KCfg K, DevState D, const uint8_t* mask, float* obs) {
  GpuCtxT<FLAT, PLAIN, BODY> c;
  if (!make_ctx(K, c)) return;
  if (mask && !mask[c.env]) return;
  __shared__ float lds_par[PR_N * BLOCK];
  stage_params(c, D, lds_par);
  LaneState<float> L = load_state<float>(c, D.base, D.leg);
  reset_finish(c, K, L, D.ring, D.ctl, D.ictl, D.legctl, D.etgp, obs);
  store_state(c, D.base, D.leg, L);
}

// ---- cached restart (etg_step_autoreset).  A launch lasts as long as its slowest wave, and with auto-reset
// some wave restarts a robot in nearly every launch; recomputing reset_finish16 there (first ETG action, IK, foot kinematics,
// rpy reference, first observation: ~1200 instructions) costs the whole batch ~3 us per step.  What reset_finish16 produces
// depends only on the settled state, the robot's parameters and its ETG weights, so etg_reset keeps it per robot -- in rows
// FIN_* of the block behind D.cache_off (rows 0, 1 are the offsets the cached settle ran at) -- and the in-kernel restart
// copies it back.  Anything that changes an input clears the robot's FIN_OK flag (etg_set_params, etg_set_heightfield,
// etg_set_reset_offsets); the restart then recomputes as before.  Both lane mappings share the SoA state layout, and this cache.
enum { FIN_OBS = 2, FIN_RPY = FIN_OBS + ETG_OBS_DIM, FIN_FWX = FIN_RPY + 3, FIN_OK = FIN_FWX + 4, FIN_ROWS = FIN_OK + 1 };
#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void __launch_bounds__(256) k_fin_store(KCfg K, DevState D, const uint8_t* mask, const float* obs) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = K.n_env;
  if (env >= N || (mask && !mask[env])) return;
  float* fin = D.cache_off;
  for (int k = 0; k < ETG_OBS_DIM; k++) fin[(size_t)(FIN_OBS + k) * N + env] = obs[(size_t)env * ETG_OBS_DIM + k];
  for (int k = 0; k < 3; k++) fin[(size_t)(FIN_RPY + k) * N + env] = D.ctl[(size_t)(CT_FIRST_RPY + k) * N + env];
  for (int leg = 0; leg < 4; leg++) fin[(size_t)(FIN_FWX + leg) * N + env] = D.legctl[(size_t)LC_LAST_FOOT_X * 4 * N + 4 * env + leg];
  fin[(size_t)FIN_OK * N + env] = 1.0f;
}
// motor strength ratios (etg_set_motor_strength): par[PR_STR + j][4 env + leg] = ratios[env][3 leg + j], or 1 when ratios is null
__global__ void __launch_bounds__(256) k_set_strength(KCfg K, DevState D, const float* ratios, const uint8_t* mask) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int NL = 4 * K.n_env;
  if (col >= NL) return;
  const int env = col >> 2, leg = col & 3;
  if (mask && !mask[env]) return;
  for (int j = 0; j < 3; j++) D.par[(size_t)(PR_STR + j) * NL + col] = ratios ? ratios[(size_t)env * ETG_NUM_MOTORS + 3 * leg + j] : 1.0f;
  if (leg == 0) {   // the reset settle runs under the motor model: the robot's cached settle and cached restart are stale
    D.cache_ok[env] = 0;
    D.cache_off[(size_t)FIN_OK * K.n_env + env] = 0.0f;
  }
}

__global__ void __launch_bounds__(256) k_fin_clear(KCfg K, DevState D, const uint8_t* mask) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= K.n_env || (mask && !mask[env])) return;
  D.cache_off[(size_t)FIN_OK * K.n_env + env] = 0.0f;
}
#endif
// reset_finish from the cache (4 lanes per robot: lane = leg): same stores, no arithmetic
template <class Ctx>
__device__ __forceinline__ void restart_from_cache4(const Ctx& c, const KCfg& K, LaneState<float>& L, float* ctl, int* ictl, float* legctl,
                                                    const float* fin, float* obs) {
  const int N = K.n_env;
  L.energy = 0.0f;
  c.st_env_i(ictl, IC_STEP, 0);
  c.st_env_i(ictl, IC_TICK, K.settle_ticks);
  c.st_env_i(ictl, IC_HAS_LAST, 0);
  c.st_env(ctl, CT_RET, 0.0f); c.st_env(ctl, CT_LEN, 0.0f); c.st_env(ctl, CT_ALIVE, 1.0f);
  c.st_env(ctl, CT_LAST_BASE + 0, L.p.x); c.st_env(ctl, CT_LAST_BASE + 1, L.p.y); c.st_env(ctl, CT_LAST_BASE + 2, L.p.z);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float pose = c.par(PR_POSE + j);
    c.st_lane(legctl, LC_LAST_QDES + j, pose);
    c.st_lane(legctl, LC_FX0 + j, pose); c.st_lane(legctl, LC_FX1 + j, pose);
    c.st_lane(legctl, LC_FY0 + j, pose); c.st_lane(legctl, LC_FY1 + j, pose);
  }
  c.st_lane(legctl, LC_LAST_FOOT_X, fin[(size_t)(FIN_FWX + c.lane) * N + c.env]);
#pragma unroll
  for (int k = 0; k < 3; k++) c.st_env(ctl, CT_FIRST_RPY + k, fin[(size_t)(FIN_RPY + k) * N + c.env]);
  for (int k = c.lane; k < ETG_OBS_DIM; k += 4) obs[(size_t)c.env * ETG_OBS_DIM + k] = fin[(size_t)(FIN_OBS + k) * N + c.env];
}

// env.step for the 16 robots of a wave (one quad each); AUTO: see step16_body.  T (AUTO only): the step's row of every robot
// goes to T.obs INSTEAD of `obs` -- the 4-lane tick sits at the 512-register budget, and a second set of row stores costs it
// scratch -- so a robot that goes on has its row of `obs` from T.obs after the launch (etg_step_autoreset_terminal: k_term_rows);
// a restarted robot's reset row goes to `obs` as without T.
template <bool FLAT, bool PLAIN, bool AUTO, int BODY = 0>
__device__ __forceinline__ void step4_body(const KCfg& K, const DevState& D, const float* action, const uint8_t* donef, float* obs,
                                           float* reward, uint8_t* done, float* info, float* lds_par, const NextDyn NX = NextDyn{nullptr, nullptr, nullptr},
                                           const TermOut T = TermOut{nullptr, nullptr}) {
  GpuCtxT<FLAT, PLAIN, BODY> c;
  if (!make_ctx(K, c)) return;
  // every cold load of the launch head is requested before the first wait (see step16_body)
  float stg[kNStaged4];
  stage4_issue(c, D, lds_par, stg);
  LaneState<float> L = load_state<float>(c, D.base, D.leg);
  StepCtl4<float> S = load_ctl4<float>(c, K, D.ctl, D.ictl, D.legctl);
  TickPar4<float> tp = load_tick_par4<float>(c);
  V3<float> fext = {0.0f, 0.0f, 0.0f};
  if (!PLAIN && K.ext_force) fext = {c.ld_env(D.ctl, CT_FEXT + 0) + c.ld_env(D.ctl, CT_PUSH + 0), c.ld_env(D.ctl, CT_FEXT + 1) + c.ld_env(D.ctl, CT_PUSH + 1),
                                     c.ld_env(D.ctl, CT_FEXT + 2) + c.ld_env(D.ctl, CT_PUSH + 2)};   // set force + random push
  float act[3], hyb[12];
  const bool hybrid = K.motor_mode == 2 && action;   // rows of 60: per motor (q_des, kp, qd_des, kd, tau_ff)
#pragma unroll
  for (int j = 0; j < 3; j++) {
    act[j] = !action ? 0.0f : hybrid ? c.ld_row_lane(action, ETG_HYBRID_DIM, 5 * j, 15) : c.ld_row_lane(action, ETG_ACT_DIM, j, 3);
#pragma unroll
    for (int k = 0; k < 4; k++) hyb[4 * j + k] = hybrid ? c.ld_row_lane(action, ETG_HYBRID_DIM, 5 * j + 1 + k, 15) : 0.0f;
  }
  const float dflag = donef ? (float)donef[c.env] : 0.0f;
  stage4_commit(c, stg);
  float r, d;
#ifdef ETG_PROFILE_PHASES
  for (int k = 0; k < 16; k++) c.prof[k] = 0;
  c.prof_last = clock64();
  long long t_begin = c.prof_last;
#endif
  control_step_core(c, K, tp, fext, L, S, D.ring, D.etgp, act, dflag, AUTO && T.obs ? T.obs : obs, r, d, info, hybrid ? hyb : nullptr);
  store_ctl4(c, K, S, D.ctl, D.ictl, D.legctl);
  if (AUTO && d > 0.5f) {   // whole quads take this branch together
    const int N = K.n_env;
    if (T.ctx) term_ctx_store(K, D, c.env, c.lane, 4, S.step_count, T.ctx);
    if (NX.ok && NX.ok[c.env]) {   // parameters prepared for the next episode: install them (the cached settle below is theirs)
      for (int k = 0; k < PR_DERIVED; k++) D.par[(size_t)k * c.NL + c.gid] = NX.par[(size_t)k * c.NL + c.gid];
      for (int k = c.lane; k < ETG_DYN_DIM; k += 4) D.dyn[(size_t)c.env * ETG_DYN_DIM + k] = NX.dyn[(size_t)c.env * ETG_DYN_DIM + k];
      __builtin_amdgcn_s_waitcnt(0);          // the quad's reads of the flag are done before its lane 0 clears it
      __builtin_amdgcn_wave_barrier();
      if (c.lane == 0) NX.ok[c.env] = 0;
      stage_params(c, D, lds_par);            // the restart below reads the staged leg parameters: the new ones
    }
    L = load_state<float>(c, D.cache_base, D.cache_leg);
    L.p.x += D.reset_off[c.env] - D.cache_off[c.env];
    L.p.y += D.reset_off[N + c.env] - D.cache_off[N + c.env];
    if (D.cache_off[(size_t)FIN_OK * N + c.env] > 0.5f) restart_from_cache4(c, K, L, D.ctl, D.ictl, D.legctl, D.cache_off, obs);
    else reset_finish(c, K, L, D.ring, D.ctl, D.ictl, D.legctl, D.etgp, obs);
    if (c.lane == 0) {
      D.ictl[(size_t)IC_PUSH_LEFT * N + c.env] = 0;
      for (int k = 0; k < 3; k++) D.ctl[(size_t)(CT_PUSH + k) * N + c.env] = 0.0f;
    }
  }
  store_state(c, D.base, D.leg, L);
#ifdef ETG_PROFILE_PHASES
  if (c.gid == 0 && info) {  // overwrite the first info row with the cycle breakdown (debug build only)
    for (int k = 0; k < 16; k++) info[k] = (float)c.prof[k];
    info[16] = (float)(clock64() - t_begin);
  }
#endif
  if (c.lane == 0) {
    reward[c.env] = r;
    done[c.env] = d > 0.5f ? 1 : 0;
  }
}
template <bool FLAT, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(BLOCK) k_step(KCfg K, DevState D, const float* action, const uint8_t* donef, float* obs,
                                                 float* reward, uint8_t* done, float* info) {
  __shared__ float lds_par[PR_N * BLOCK];
  step4_body<FLAT, PLAIN, false, BODY>(K, D, action, donef, obs, reward, done, info, lds_par);
}
template <bool FLAT, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(BLOCK) k_step_ar(KCfg K, DevState D, const float* action, const uint8_t* donef, float* obs,
                                                    float* reward, uint8_t* done, float* info, NextDyn NX, TermOut T) {
  __shared__ float lds_par[PR_N * BLOCK];
  step4_body<FLAT, PLAIN, true, BODY>(K, D, action, donef, obs, reward, done, info, lds_par, NX, T);
}

// episode returns / lengths [N] for the caller, or nulls; cyc: one slot per wavefront of the launch receiving the shader-clock
// cycles the wave spent in the kernel (etg_rollout_wave_cycles: how unevenly the sweeps load the wavefronts), or null
struct StatOut { float* ret; int* len; long long* cyc; };
// n_steps open-loop control steps per launch (rollout_steps), the 4-lanes-per-robot counterpart of k_rollout16
template <bool FLAT, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(BLOCK) k_rollout(KCfg K, DevState D, int n_steps, float* obs, StatOut so) {
  GpuCtxT<FLAT, PLAIN, BODY> c;
  if (!make_ctx(K, c)) return;
  const long long t0 = so.cyc ? clock64() : 0;
  __shared__ float lds_par[PR_N * BLOCK];
  stage_params(c, D, lds_par);
  LaneState<float> L = load_state<float>(c, D.base, D.leg);
  rollout_steps(c, K, L, D.base, D.leg, D.ring, D.ctl, D.ictl, D.legctl, D.etgp, n_steps, obs);   // (stores the state itself: stop_at_done)
  if (so.cyc && threadIdx.x == 0) so.cyc[blockIdx.x] = clock64() - t0;
  if (so.ret && c.lane == 0) {   // the last launch of a rollout hands the episode statistics to the caller itself (no extra launch)
    so.ret[c.env] = D.ctl[(size_t)CT_RET * K.n_env + c.env];
    so.len[c.env] = (int)D.ctl[(size_t)CT_LEN * K.n_env + c.env];
  }
}

// n_steps control steps over a caller-supplied action tape [n_steps][N][12] in one launch (etg_rollout_actions): the
// dynamics-identification evaluator's 2 x 100 steps of known joint targets (Dynamic_parallel_model.py:53-77) and teacher
// replays.  T: optional per-step outputs ([n_steps][N][...], null = not recorded).
struct TapeOut { float *q, *imu, *obs, *rew; uint8_t* done; };
template <bool FLAT, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(BLOCK) k_rollout_actions(KCfg K, DevState D, int n_steps, const float* actions, float* obs, TapeOut T) {
  GpuCtxT<FLAT, PLAIN, BODY> c;
  if (!make_ctx(K, c)) return;
  __shared__ float lds_par[PR_N * BLOCK];
  stage_params(c, D, lds_par);
  LaneState<float> L = load_state<float>(c, D.base, D.leg);
  StepCtl4<float> S = load_ctl4<float>(c, K, D.ctl, D.ictl, D.legctl);
  TickPar4<float> tp = load_tick_par4<float>(c);
  V3<float> fext = {0.0f, 0.0f, 0.0f};
  if (!PLAIN && K.ext_force) fext = {c.ld_env(D.ctl, CT_FEXT + 0) + c.ld_env(D.ctl, CT_PUSH + 0), c.ld_env(D.ctl, CT_FEXT + 1) + c.ld_env(D.ctl, CT_PUSH + 1),
                                     c.ld_env(D.ctl, CT_FEXT + 2) + c.ld_env(D.ctl, CT_PUSH + 2)};
  const size_t N = K.n_env;
  float reward, done;
  const bool skip = K.stop_at_done != 0;
  for (int s = 0; s < n_steps; s++) {
    const float* a = actions + (size_t)s * N * ETG_ACT_DIM;
    const float act[3] = {c.ld_row_lane(a, ETG_ACT_DIM, 0, 3), c.ld_row_lane(a, ETG_ACT_DIM, 1, 3), c.ld_row_lane(a, ETG_ACT_DIM, 2, 3)};
    const bool last = s == n_steps - 1;
    const float was_alive = S.alive;
    // (stop_at_done: the steps after a robot's episode write reward 0 / done 1 to the tape and leave its other rows alone; once
    // every robot of the wave has finished only those two are written)
    if (!skip || c.any(was_alive > 0.5f)) {
      control_step_core(c, K, tp, fext, L, S, D.ring, D.etgp, act, 0.0f, (T.obs && !last) ? T.obs + (size_t)s * N * ETG_OBS_DIM : obs, reward, done,
                        (float*)nullptr, (const float*)nullptr, last || T.obs || T.imu, T.q ? T.q + (size_t)s * N * ETG_ACT_DIM : nullptr,
                        T.imu ? T.imu + (size_t)s * N * 6 : nullptr, skip, obs);
      // (a robot that ends mid-launch leaves its last row in the tape AND in `obs`; recorded rows and sensor noise exclude each
      // other -- etg_rollout_actions refuses the combination -- so with noise on every row in `obs` notes its stream position)
      if (skip) rollout_dead_store(c, K, L, was_alive, done, last, true, (int)K.noise_call + s, D.base, D.leg, D.ictl);
    } else {
      reward = 0.0f; done = 1.0f;
    }
    if (c.lane == 0) {
      if (T.rew) T.rew[(size_t)s * N + c.env] = reward;
      if (T.done) T.done[(size_t)s * N + c.env] = done > 0.5f ? 1 : 0;
    }
  }
  store_ctl4(c, K, S, D.ctl, D.ictl, D.legctl);
  rollout_store(c, K, L, S.alive, D.base, D.leg);
}

// ====================================================================== 16 lanes per robot
// One robot = one 16-lane DPP row (etg_core16.h): lane r = 4*leg + sub.  A workgroup is still one
// wave64 = 4 robots; 4096 robots -> 1024 workgroups = one wave on every SIMD of the chip.
constexpr int LDS16_FIELDS = PR_N;  // one LDS column per lane, indexed by PR_* (only the staged fields are filled)

struct GpuCtx16 {
  int env, r, leg, sub, sc, tid, N, NL;
  size_t col;        // 4*env + leg : column of the leg-level SoA arrays
  const float* lds;  // this lane's LDS column
  const float* gpar; // D.par: the tick constants are read from it directly (tpar*)
  int row_base = 0;  // first robot of the [*, rowlen] row buffers (obs tile in LDS: the workgroup's first robot)
#ifdef ETG_TRACE_TICKS
  mutable int trace_i = 0;
  __device__ __forceinline__ void trace_index(int i) const { trace_i = i; }
  __device__ __forceinline__ void trace_tick(const KCfg& K, const float* v) const {
    if (!K.trace || trace_i >= 16) return;
    float* row = K.trace + (((size_t)env * 16 + trace_i) * 16 + r) * 10;
    for (int k = 0; k < 10; k++) row[k] = v[k];
  }
#endif
  mutable bool gate = true;   // store gate: see GpuCtx
  __device__ __forceinline__ void set_gate(bool on) const { gate = on; }
  __device__ __forceinline__ void open_gate() const { gate = true; }
  __device__ __forceinline__ int sel_i(bool m, int a, int b) const { return m ? a : b; }
  // The lane's coordinates through an empty asm: everything derived from them after this point (the tick's lane masks, per-lane
  // constants selected from the config block: ~60 registers) is computed HERE again instead of being hoisted out of the caller's
  // loop -- the per-wave closed-loop kernel calls it at the top of every control step, so that none of it lives across the
  // policy tile (where the allocator would spill it to scratch).
  __device__ __forceinline__ void launder_lane() {
    asm volatile("" : "+v"(r), "+v"(leg), "+v"(sub), "+v"(sc));
    int lo = (int)col, e = env;             // (the array columns too: addresses are formed where they are used, not kept from the kernel's head)
    asm volatile("" : "+v"(lo), "+v"(e));
    col = (size_t)(unsigned)lo;
    env = e;
  }
  __device__ __forceinline__ float jointf() const { return sub < 3 ? 1.0f : 0.0f; }
  __device__ __forceinline__ bool sub_is(int j) const { return sub == j; }
  __device__ __forceinline__ bool leg_is(int j) const { return leg == j; }
  __device__ __forceinline__ bool any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0ull; }
  // the wave-uniform tests of the body paths work on the wave mask of a compare: "any lane", "any lane of leg lp (in any robot
  // of the wave)" are one scalar AND against a constant each
  __device__ __forceinline__ bool any_body(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0ull; }
  // the wave mask folded to 32 bits (a leg's four lanes sit at the same bits of both halves): a leg's test is ONE s_and_b32
  // against a 32-bit literal that sets SCC (a 64-bit mask needs two ANDs and a compare)
  __device__ __forceinline__ unsigned body_mask(bool b) const {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(b);
    return (unsigned)m | (unsigned)(m >> 32);
  }
  __device__ __forceinline__ bool mask_any(unsigned m) const { return m != 0u; }
  __device__ __forceinline__ bool mask_leg(unsigned m, int lp) const { return (m & (0x000F000Fu << (4 * lp))) != 0u; }
  __device__ __forceinline__ unsigned uniform_bits(unsigned v) const { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }   // a wave-uniform value, kept in an SGPR
  // "does any lane of MY robot (16-lane row) see b?" from the wave mask of the compare
  __device__ __forceinline__ bool vote_robot(unsigned long long m) const {
    const unsigned f = (tid & 16) ? 0xFFFF0000u : 0x0000FFFFu;
    return ((tid & 32) ? ((unsigned)(m >> 32) & f) : ((unsigned)m & f)) != 0u;
  }
  // the residual rule's votes (etg_core16.h: sweep_and_test): one wave mask per compare, OR-ed as scalars
  // (the builtin on the i1 itself: HIP's __any / __ballot take an int, and the compare's wave mask went through a
  // v_cndmask 0/1 + v_cmp_ne + a wait state on its way in -- three issue slots per sweep)
  __device__ __forceinline__ unsigned long long vote(bool b) const { return __builtin_amdgcn_ballot_w64(b); }
  __device__ __forceinline__ unsigned long long vote_or(unsigned long long a, unsigned long long b) const { return a | b; }
  __device__ __forceinline__ bool vote_wave(unsigned long long m) const { return m != 0ull; }
  __device__ __forceinline__ void fence() const { asm volatile(""); }   // keeps two tests two branches
  __device__ __forceinline__ int uniform_int(float a) const { return (int)a; }
  __device__ __forceinline__ float par(int k) const { return lds[k * 64]; }
  __device__ __forceinline__ float par_joint(int base) const { return lds[(base + sc) * 64]; }
  __device__ __forceinline__ float tpar(int k) const { return gpar[(size_t)k * NL + col]; }
  __device__ __forceinline__ float tpar_joint(int base) const { return gpar[(size_t)(base + sc) * NL + col]; }
  __device__ __forceinline__ float tpar_link(int k) const { return sub < 3 ? gpar[(size_t)(PR_LINK + 10 * sub + k) * NL + col] : 0.0f; }
  // ---- quad (= leg) exchanges
  __device__ __forceinline__ float qb(float a, int j) const {
    switch (j) { case 0: return dpp_<0x00>(a); case 1: return dpp_<0x55>(a); case 2: return dpp_<0xAA>(a); default: return dpp_<0xFF>(a); }
  }
  __device__ __forceinline__ float qup1(float a) const { return dpp_<0xF9>(a); }     // quad_perm [1,2,3,3]
  __device__ __forceinline__ float qup2(float a) const { return dpp_<0xFE>(a); }     // quad_perm [2,3,3,3]
  __device__ __forceinline__ float qdn1(float a) const { return dpp_<0x93>(a); }     // quad_perm [3,0,1,2]
  __device__ __forceinline__ float qdn2(float a) const { return dpp_<0x4F>(a); }     // quad_perm [3,3,0,1]
  __device__ __forceinline__ float qswap12(float a) const { return dpp_<0xD8>(a); }  // quad_perm [0,2,1,3]
  __device__ __forceinline__ float qsum(float a) const { float t = a + dpp_<0xB1>(a); return t + dpp_<0x4E>(t); }
  // ---- row (= robot) exchanges: xor1, xor2, row_half_mirror, row_mirror -- order-symmetric, so the
  // result is bit-identical on the 16 lanes
  // six row sums advanced stage by stage: every DPP reads a value written six instructions earlier
  __device__ __forceinline__ void sum16xn(float* v, int n) const {   // n is a compile-time constant at the call sites
#pragma unroll
    for (int k = 0; k < n; k++) v[k] = v[k] + dpp_<0xB1>(v[k]);
#pragma unroll
    for (int k = 0; k < n; k++) v[k] = v[k] + dpp_<0x4E>(v[k]);
#pragma unroll
    for (int k = 0; k < n; k++) v[k] = v[k] + dpp_<0x141>(v[k]);
#pragma unroll
    for (int k = 0; k < n; k++) v[k] = v[k] + dpp_<0x140>(v[k]);
  }
  __device__ __forceinline__ void sum16x6(float* v) const {
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = v[k] + dpp_<0xB1>(v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = v[k] + dpp_<0x4E>(v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = v[k] + dpp_<0x141>(v[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = v[k] + dpp_<0x140>(v[k]);
  }
  __device__ __forceinline__ float sum16(float a) const {
    float t = a + dpp_<0xB1>(a); t = t + dpp_<0x4E>(t); t = t + dpp_<0x141>(t); return t + dpp_<0x140>(t);
  }
  __device__ __forceinline__ float max16(float a) const {
    float t = fmaxf(a, dpp_<0xB1>(a)); t = fmaxf(t, dpp_<0x4E>(t)); t = fmaxf(t, dpp_<0x141>(t)); return fmaxf(t, dpp_<0x140>(t));
  }
  __device__ __forceinline__ float rbcast(float a, int r0) const {  // row_newbcast:r0 (constant after unrolling)
    switch (r0) {
      case 0: return dpp_<0x150>(a); case 1: return dpp_<0x151>(a); case 2: return dpp_<0x152>(a); case 3: return dpp_<0x153>(a);
      case 4: return dpp_<0x154>(a); case 5: return dpp_<0x155>(a); case 6: return dpp_<0x156>(a); case 7: return dpp_<0x157>(a);
      case 8: return dpp_<0x158>(a); case 9: return dpp_<0x159>(a); case 10: return dpp_<0x15A>(a); case 11: return dpp_<0x15B>(a);
      case 12: return dpp_<0x15C>(a); case 13: return dpp_<0x15D>(a); case 14: return dpp_<0x15E>(a); default: return dpp_<0x15F>(a);
    }
  }
  // value of the same sub-lane in leg (leg + kk) mod 4: row_ror:n delivers lane (i - n) mod 16
  __device__ __forceinline__ float legrot(float a, int kk) const {
    switch (kk) { case 0: return a; case 1: return dpp_<0x12C>(a); case 2: return dpp_<0x128>(a); default: return dpp_<0x124>(a); }
  }
  __device__ __forceinline__ void quad_outer(float a, float b, float* acc) const {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 v = {acc[0], acc[1], acc[2], acc[3]};
    v = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, v, 0, 0, 0);
    acc[0] = v[0]; acc[1] = v[1]; acc[2] = v[2]; acc[3] = v[3];
  }
  // ---- four Gram columns per matrix instruction (gram16.h; etg_core16.h: kGramMfma): c[lp][e] = sum over the six base
  // coordinates of a[k]@(lane 4 lp + e of the robot's row) * b[k] -- the 16 columns of a row set in one block of 24
  // instructions, bit for bit what 16 chains of one product and five fmac_rbcast compute
  typedef gram4_t gram_t;
  __device__ __forceinline__ void gram16(gram_t (&c)[4], const float* a, const float* b) const { gram16_block(c, gram4_seed(), a, b); }
  // the broadcast sources that remain DPP operands once the Z vectors go through the matrix pipe (dpp_ready10 without Z)
  __device__ __forceinline__ void dpp_ready4(float* hj, float* lam) const { asm volatile("s_nop 1" : "+v"(hj[0]), "+v"(hj[1]), "+v"(hj[2]), "+v"(lam[0])); }
  // ---- fused broadcast-multiply-accumulate: acc += x@lane(r0 of the row / j of the quad) * y in ONE VOP2-DPP
  // instruction.  The compiler's DPP combiner only folds v_mov_dpp into mul/add (FMAs are still VOP3 when it
  // runs), so the FMA form is spelled out.  HAZARD: the hardware wants 2 wait states between the VALU write
  // of x and a DPP read of it, and the compiler does not see into the asm -- callers pass an x that went
  // through dpp_ready() (one s_nop 1 for a whole group of sources).
#define ETG_FMAC_DPP(CTRL) asm("v_fmac_f32_dpp %0, %1, %2 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(acc) : "v"(x), "v"(y))
  __device__ __forceinline__ void fmac_rbcast(float& acc, float x, float y, int r0) const {
    switch (r0) {
      case 0: ETG_FMAC_DPP("row_newbcast:0"); break;   case 1: ETG_FMAC_DPP("row_newbcast:1"); break;
      case 2: ETG_FMAC_DPP("row_newbcast:2"); break;   case 3: ETG_FMAC_DPP("row_newbcast:3"); break;
      case 4: ETG_FMAC_DPP("row_newbcast:4"); break;   case 5: ETG_FMAC_DPP("row_newbcast:5"); break;
      case 6: ETG_FMAC_DPP("row_newbcast:6"); break;   case 7: ETG_FMAC_DPP("row_newbcast:7"); break;
      case 8: ETG_FMAC_DPP("row_newbcast:8"); break;   case 9: ETG_FMAC_DPP("row_newbcast:9"); break;
      case 10: ETG_FMAC_DPP("row_newbcast:10"); break; case 11: ETG_FMAC_DPP("row_newbcast:11"); break;
      case 12: ETG_FMAC_DPP("row_newbcast:12"); break; case 13: ETG_FMAC_DPP("row_newbcast:13"); break;
      case 14: ETG_FMAC_DPP("row_newbcast:14"); break; default: ETG_FMAC_DPP("row_newbcast:15"); break;
    }
  }
  __device__ __forceinline__ void fmac_qb(float& acc, float x, float y, int j) const {
    switch (j) {
      case 0: ETG_FMAC_DPP("quad_perm:[0,0,0,0]"); break; case 1: ETG_FMAC_DPP("quad_perm:[1,1,1,1]"); break;
      case 2: ETG_FMAC_DPP("quad_perm:[2,2,2,2]"); break; default: ETG_FMAC_DPP("quad_perm:[3,3,3,3]"); break;
    }
  }
  // the 12 warm-start terms in one asm block: consecutive inline-asm statements that accumulate into one register
  // get a compiler-inserted wait state each (it cannot see that the accumulator is not the DPP operand)
  __device__ __forceinline__ void fmac_rbcast12(float& acc, float x, const float* a) const {
#define ETG_L(R, N) "v_fmac_f32_dpp %0, %1, %" #N " row_newbcast:" #R " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
    asm(ETG_L(0, 2) ETG_L(1, 3) ETG_L(2, 4) ETG_L(4, 5) ETG_L(5, 6) ETG_L(6, 7) ETG_L(8, 8) ETG_L(9, 9) ETG_L(10, 10)
        ETG_L(12, 11) ETG_L(13, 12) ETG_L(14, 13)
        : "+&v"(acc)
        : "v"(x), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
          "v"(a[10]), "v"(a[11]));
#undef ETG_L
  }
  // body friction rows (etg_core16.h: body_friction): acc + sum over the 16 first rows of x@lane * a[lane] + sum over the eight
  // second rows (the t1 / t2 lanes of the four legs) of y@lane * b[2 leg + t].  24 broadcast-FMAs into ONE register would be a
  // dependent chain (a lone wave sits out every link): four partial sums advance side by side and are added at the end.
  __device__ __forceinline__ float row2_velocity(float acc, float x, const float* a, float y, const float* b) const {
    float p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#define ETG_L(ACC, SRC, R, N) "v_fmac_f32_dpp %" #ACC ", %" #SRC ", %" #N " row_newbcast:" #R " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
    asm(ETG_L(0, 4, 0, 6) ETG_L(1, 4, 1, 7) ETG_L(2, 4, 2, 8) ETG_L(3, 4, 3, 9) ETG_L(0, 4, 4, 10) ETG_L(1, 4, 5, 11) ETG_L(2, 4, 6, 12) ETG_L(3, 4, 7, 13)
        ETG_L(0, 4, 8, 14) ETG_L(1, 4, 9, 15) ETG_L(2, 4, 10, 16) ETG_L(3, 4, 11, 17) ETG_L(0, 4, 12, 18) ETG_L(1, 4, 13, 19) ETG_L(2, 4, 14, 20) ETG_L(3, 4, 15, 21)
        ETG_L(0, 5, 1, 22) ETG_L(1, 5, 2, 23) ETG_L(2, 5, 5, 24) ETG_L(3, 5, 6, 25) ETG_L(0, 5, 9, 26) ETG_L(1, 5, 10, 27) ETG_L(2, 5, 13, 28) ETG_L(3, 5, 14, 29)
        : "+&v"(acc), "+&v"(p1), "+&v"(p2), "+&v"(p3)     // (early-clobber: an input holding the same VALUE as an accumulator's start --
                                                            // y = 0 and p3 = 0 -- must not share its register: it is read after the writes)
        : "v"(x), "v"(y), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
          "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]),
          "v"(b[5]), "v"(b[6]), "v"(b[7]));
#undef ETG_L
    return (acc + p1) + (p2 + p3);
  }
#undef ETG_FMAC_DPP
  // ---- the contact solve's sweep, hand-scheduled (etg_core16.h: pgs_sweep; kAsmSweep).  The sweep is one serial chain --
  // candidate -> broadcast -> apply, row after row -- and every broadcast reads a register the instruction before wrote: the
  // hardware wants 2 wait states between a VALU write and a DPP read of it.  The compiler's version spends a v_mov_b32_dpp plus
  // an s_nop 1 per broadcast (17 + 16 of 104 instructions, 120 issue slots per sweep); here the broadcast is the DPP operand
  // of the applying v_fmac itself and the owner's own impulse update sits in one of the two wait states: 5 slots per normal row,
  // 16 per friction pair, 84 per sweep.  Same arithmetic as the C++ statement in pgs_sweep (which the emulation, the body-row
  // and the pyramid instantiations keep).
#define ETG_DPPC " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
  __device__ __forceinline__ void pgs_normals(float& lam, float& u, float iA, float c0, const float (&A)[4][3], const float* mk0) const {
    float t, d;
#define ETG_ROW(LP, AOP, MOP)                                                    \
    "v_fma_f32 %[t], -%[u], %[iA], %[c0]\n"        /* t = c0 - u / A            */ \
    "v_max_f32_e64 %[d], -%[lam], %[t]\n"          /* d = max(-lam, t)          */ \
    "v_fmac_f32_e32 %[lam], %[" MOP "], %[d]\n"    /* the owner commits         */ \
    "s_nop 0\n"                                                                    \
    "v_fmac_f32_dpp %[u], %[d], %[" AOP "] row_newbcast:" #LP ETG_DPPC
    asm(ETG_ROW(0, "a0", "m0") ETG_ROW(4, "a1", "m1") ETG_ROW(8, "a2", "m2") ETG_ROW(12, "a3", "m3")
        : [lam] "+&v"(lam), [u] "+&v"(u), [t] "=&v"(t), [d] "=&v"(d)
        : [iA] "v"(iA), [c0] "v"(c0), [a0] "v"(A[0][0]), [a1] "v"(A[1][0]), [a2] "v"(A[2][0]), [a3] "v"(A[3][0]),
          [m0] "v"(mk0[0]), [m1] "v"(mk0[1]), [m2] "v"(mk0[2]), [m3] "v"(mk0[3]));
  }
  // the same with the four body normal rows (aux lanes) after the feet's: Bullet's order -- every normal row, then friction
  __device__ __forceinline__ void pgs_normals_body(float& lam, float& u, float iA, float c0, const float (&A)[4][3], const float* Ak,
                                                   const float* mk0, const float* mk3) const {
    float t, d;
    asm(ETG_ROW(0, "a0", "m0") ETG_ROW(4, "a1", "m1") ETG_ROW(8, "a2", "m2") ETG_ROW(12, "a3", "m3")
        ETG_ROW(3, "k0", "n0") ETG_ROW(7, "k1", "n1") ETG_ROW(11, "k2", "n2") ETG_ROW(15, "k3", "n3")
        : [lam] "+&v"(lam), [u] "+&v"(u), [t] "=&v"(t), [d] "=&v"(d)
        : [iA] "v"(iA), [c0] "v"(c0), [a0] "v"(A[0][0]), [a1] "v"(A[1][0]), [a2] "v"(A[2][0]), [a3] "v"(A[3][0]),
          [m0] "v"(mk0[0]), [m1] "v"(mk0[1]), [m2] "v"(mk0[2]), [m3] "v"(mk0[3]),
          [k0] "v"(Ak[0]), [k1] "v"(Ak[1]), [k2] "v"(Ak[2]), [k3] "v"(Ak[3]),
          [n0] "v"(mk3[0]), [n1] "v"(mk3[1]), [n2] "v"(mk3[2]), [n3] "v"(mk3[3]));
  }
#undef ETG_ROW
  // The sweeps of a tick with body rows track the velocity `u2` of the SECOND row set (the body contacts' friction rows,
  // etg_core16.h: finish_tick) through every phase: each impulse change is applied to u2 as well, by one more broadcast-FMA
  // that sits in a wait state the row needs anyway (the change of row i is applied to u2 while row i + 1 waits for its own
  // broadcast: the two changes alternate between the registers dA / dB).  8 rows: 41 issue slots, as many as without u2.
  // The block ends with the two quad broadcasts the friction phases start from -- the leg's foot normal impulse `lnq` and body
  // normal impulse `lbn` -- where the last rows' tails are their wait states (after the block the compiler fences each with an
  // s_nop 1: it does not see into the asm).
  __device__ __forceinline__ void pgs_normals_body2(float& lam, float& u, float& u2, float iA, float c0, const float (&A)[4][3],
                                                    const float* Ak, const float* mk0, const float* mk3, const float* bn, float& lnq,
                                                    float& lbn) const {
    float t, dA, dB;
#define ETG_ROW2(D, LP, AOP, MOP, FILL)                                            \
    "v_fma_f32 %[t], -%[u], %[iA], %[c0]\n"                                        \
    "v_max_f32_e64 %[" D "], -%[lam], %[t]\n"                                      \
    "v_fmac_f32_e32 %[lam], %[" MOP "], %[" D "]\n"                                \
    FILL                                                                           \
    "v_fmac_f32_dpp %[u], %[" D "], %[" AOP "] row_newbcast:" #LP ETG_DPPC
#define ETG_U2(D, LP, BOP) "v_fmac_f32_dpp %[u2], %[" D "], %[" BOP "] row_newbcast:" #LP ETG_DPPC
    asm(ETG_ROW2("dA", 0, "a0", "m0", "s_nop 0\n")
        ETG_ROW2("dB", 4, "a1", "m1", ETG_U2("dA", 0, "b0"))
        ETG_ROW2("dA", 8, "a2", "m2", ETG_U2("dB", 4, "b1"))
        ETG_ROW2("dB", 12, "a3", "m3", ETG_U2("dA", 8, "b2"))
        ETG_ROW2("dA", 3, "k0", "n0", ETG_U2("dB", 12, "b3"))
        ETG_ROW2("dB", 7, "k1", "n1", ETG_U2("dA", 3, "b4"))
        ETG_ROW2("dA", 11, "k2", "n2", ETG_U2("dB", 7, "b5"))
        ETG_ROW2("dB", 15, "k3", "n3", ETG_U2("dA", 11, "b6"))
        ETG_U2("dB", 15, "b7")
        "v_mov_b32_dpp %[lnq], %[lam] quad_perm:[0,0,0,0]" ETG_DPPC
        "v_mov_b32_dpp %[lbn], %[lam] quad_perm:[3,3,3,3]" ETG_DPPC
        : [lam] "+&v"(lam), [u] "+&v"(u), [u2] "+&v"(u2), [t] "=&v"(t), [dA] "=&v"(dA), [dB] "=&v"(dB), [lnq] "=&v"(lnq), [lbn] "=&v"(lbn)
        : [iA] "v"(iA), [c0] "v"(c0), [a0] "v"(A[0][0]), [a1] "v"(A[1][0]), [a2] "v"(A[2][0]), [a3] "v"(A[3][0]),
          [m0] "v"(mk0[0]), [m1] "v"(mk0[1]), [m2] "v"(mk0[2]), [m3] "v"(mk0[3]),
          [k0] "v"(Ak[0]), [k1] "v"(Ak[1]), [k2] "v"(Ak[2]), [k3] "v"(Ak[3]),
          [n0] "v"(mk3[0]), [n1] "v"(mk3[1]), [n2] "v"(mk3[2]), [n3] "v"(mk3[3]),
          [b0] "v"(bn[0]), [b1] "v"(bn[1]), [b2] "v"(bn[2]), [b3] "v"(bn[3]), [b4] "v"(bn[4]), [b5] "v"(bn[5]), [b6] "v"(bn[6]), [b7] "v"(bn[7]));
#undef ETG_ROW2
  }
  // friction pairs of the four feet on the disc: iA / lim already carry the "normal impulse > 0" condition (iA = 0 and
  // lim = 1e30 where it does not hold: the candidate is the current impulse, the scale 1, the change an exact zero)
  __device__ __forceinline__ void pgs_tangents_disc(float& lam, float& u, float iA, float lim, const float (&A)[4][3], const float* mt) const {
    float lc, sq, sc, dl;
#define ETG_PAIR(R1, R2, A1, A2, MOP)                                                                  \
    "v_fma_f32 %[lc], -%[u], %[iA], %[lam]\n"                /* candidate of this lane's row        */ \
    "v_fmaak_f32 %[sq], %[lc], %[lc], 0x0da24260\n"          /* lc^2 + 1e-30                       */ \
    "s_nop 1\n"                                                                                        \
    "v_add_f32_dpp %[sq], %[sq], %[sq] quad_perm:[0,2,1,3]" ETG_DPPC /* + the other row's           */ \
    "v_rsq_f32_e32 %[sq], %[sq]\n"                                                                     \
    "s_nop 0\n"                                                                                        \
    "v_mul_f32_e32 %[sc], %[lim], %[sq]\n"                                                             \
    "v_min_f32_e32 %[sc], 1.0, %[sc]\n"                      /* projection on the disc             */ \
    "v_fma_f32 %[dl], %[lc], %[sc], -%[lam]\n"                                                         \
    "v_fmac_f32_e32 %[lam], %[" MOP "], %[dl]\n"             /* the owners commit                  */ \
    "s_nop 0\n"                                                                                        \
    "v_fmac_f32_dpp %[u], %[dl], %[" A1 "] row_newbcast:" #R1 ETG_DPPC                                  \
    "v_fmac_f32_dpp %[u], %[dl], %[" A2 "] row_newbcast:" #R2 ETG_DPPC
    asm(ETG_PAIR(1, 2, "a01", "a02", "m0") ETG_PAIR(5, 6, "a11", "a12", "m1") ETG_PAIR(9, 10, "a21", "a22", "m2") ETG_PAIR(13, 14, "a31", "a32", "m3")
        : [lam] "+&v"(lam), [u] "+&v"(u), [lc] "=&v"(lc), [sq] "=&v"(sq), [sc] "=&v"(sc), [dl] "=&v"(dl)
        : [iA] "v"(iA), [lim] "v"(lim), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a11] "v"(A[1][1]), [a12] "v"(A[1][2]), [a21] "v"(A[2][1]),
          [a22] "v"(A[2][2]), [a31] "v"(A[3][1]), [a32] "v"(A[3][2]), [m0] "v"(mt[0]), [m1] "v"(mt[1]), [m2] "v"(mt[2]), [m3] "v"(mt[3]));
#undef ETG_PAIR
  }
  // the same with `u2` tracked (pgs_normals_body2): the two changes of pair p reach u2 in the two wait states pair p + 1 spends
  // between its squares and their exchange
  __device__ __forceinline__ void pgs_tangents_disc2(float& lam, float& u, float& u2, float iA, float lim, const float (&A)[4][3],
                                                     const float* mt, const float* bt) const {
    float lc, sq, sc, dA, dB;
#define ETG_PAIR2(D, R1, R2, A1, A2, MOP, FILL)                                                        \
    "v_fma_f32 %[lc], -%[u], %[iA], %[lam]\n"                                                          \
    "v_fmaak_f32 %[sq], %[lc], %[lc], 0x0da24260\n"                                                    \
    FILL                                                                                               \
    "v_add_f32_dpp %[sq], %[sq], %[sq] quad_perm:[0,2,1,3]" ETG_DPPC                                   \
    "v_rsq_f32_e32 %[sq], %[sq]\n"                                                                     \
    "s_nop 0\n"                                                                                        \
    "v_mul_f32_e32 %[sc], %[lim], %[sq]\n"                                                             \
    "v_min_f32_e32 %[sc], 1.0, %[sc]\n"                                                                \
    "v_fma_f32 %[" D "], %[lc], %[sc], -%[lam]\n"                                                      \
    "v_fmac_f32_e32 %[lam], %[" MOP "], %[" D "]\n"                                                    \
    "s_nop 0\n"                                                                                        \
    "v_fmac_f32_dpp %[u], %[" D "], %[" A1 "] row_newbcast:" #R1 ETG_DPPC                              \
    "v_fmac_f32_dpp %[u], %[" D "], %[" A2 "] row_newbcast:" #R2 ETG_DPPC
    asm(ETG_PAIR2("dA", 1, 2, "a01", "a02", "m0", "s_nop 1\n")
        ETG_PAIR2("dB", 5, 6, "a11", "a12", "m1", ETG_U2("dA", 1, "b0") ETG_U2("dA", 2, "b1"))
        ETG_PAIR2("dA", 9, 10, "a21", "a22", "m2", ETG_U2("dB", 5, "b2") ETG_U2("dB", 6, "b3"))
        ETG_PAIR2("dB", 13, 14, "a31", "a32", "m3", ETG_U2("dA", 9, "b4") ETG_U2("dA", 10, "b5"))
        ETG_U2("dB", 13, "b6") ETG_U2("dB", 14, "b7")
        : [lam] "+&v"(lam), [u] "+&v"(u), [u2] "+&v"(u2), [lc] "=&v"(lc), [sq] "=&v"(sq), [sc] "=&v"(sc), [dA] "=&v"(dA), [dB] "=&v"(dB)
        : [iA] "v"(iA), [lim] "v"(lim), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a11] "v"(A[1][1]), [a12] "v"(A[1][2]), [a21] "v"(A[2][1]),
          [a22] "v"(A[2][2]), [a31] "v"(A[3][1]), [a32] "v"(A[3][2]), [m0] "v"(mt[0]), [m1] "v"(mt[1]), [m2] "v"(mt[2]), [m3] "v"(mt[3]),
          [b0] "v"(bt[0]), [b1] "v"(bt[1]), [b2] "v"(bt[2]), [b3] "v"(bt[3]), [b4] "v"(bt[4]), [b5] "v"(bt[5]), [b6] "v"(bt[6]), [b7] "v"(bt[7]));
#undef ETG_PAIR2
#undef ETG_U2
  }
  // ONE friction pair of a body contact (second rows of leg lp, on its t1 / t2 lanes): the pair of pgs_tangents_disc on (lam2, u2),
  // its two changes applied to the second rows' velocity u2 AND to the first rows' u (etg_core16.h: body_friction)
  __device__ __forceinline__ void pgs_pair_body(float& lam2, float& u2, float& u, float iA, float lim, float at0, float at1, float bb0,
                                                float bb1, float mk, int lp) const {
    float lc, sq, sc, dl;
#define ETG_PAIRB(R1, R2)                                                                             \
    asm("v_fma_f32 %[lc], -%[u2], %[iA], %[lam]\n"                                                      \
        "v_fmaak_f32 %[sq], %[lc], %[lc], 0x0da24260\n"                                                 \
        "s_nop 1\n"                                                                                     \
        "v_add_f32_dpp %[sq], %[sq], %[sq] quad_perm:[0,2,1,3]" ETG_DPPC                                \
        "v_rsq_f32_e32 %[sq], %[sq]\n"                                                                  \
        "s_nop 0\n"                                                                                     \
        "v_mul_f32_e32 %[sc], %[lim], %[sq]\n"                                                          \
        "v_min_f32_e32 %[sc], 1.0, %[sc]\n"                                                             \
        "v_fma_f32 %[dl], %[lc], %[sc], -%[lam]\n"                                                      \
        "v_fmac_f32_e32 %[lam], %[mk], %[dl]\n"                                                         \
        "s_nop 0\n"                                                                                     \
        "v_fmac_f32_dpp %[u], %[dl], %[at0] row_newbcast:" #R1 ETG_DPPC                                 \
        "v_fmac_f32_dpp %[u2], %[dl], %[bb0] row_newbcast:" #R1 ETG_DPPC                                \
        "v_fmac_f32_dpp %[u], %[dl], %[at1] row_newbcast:" #R2 ETG_DPPC                                 \
        "v_fmac_f32_dpp %[u2], %[dl], %[bb1] row_newbcast:" #R2 ETG_DPPC                                \
        : [lam] "+&v"(lam2), [u2] "+&v"(u2), [u] "+&v"(u), [lc] "=&v"(lc), [sq] "=&v"(sq), [sc] "=&v"(sc), [dl] "=&v"(dl)           \
        : [iA] "v"(iA), [lim] "v"(lim), [at0] "v"(at0), [at1] "v"(at1), [bb0] "v"(bb0), [bb1] "v"(bb1), [mk] "v"(mk))
    switch (lp) { case 0: ETG_PAIRB(1, 2); break; case 1: ETG_PAIRB(5, 6); break; case 2: ETG_PAIRB(9, 10); break; default: ETG_PAIRB(13, 14); break; }
#undef ETG_PAIRB
  }
#ifndef ETG_NO_ASM_SWEEP
  // ---- the residual-rule loop of a tick with body rows as ONE scheduled stream (etg_core16.h: solve; kSweepStream): the rows of
  // pgs_normals_body2, pgs_tangents_disc2 and pgs_pair_body, instruction for instruction, with everything sweep_and_test does
  // AROUND them -- copies, grip selects, the body pairs' constants and leg tests, the residual votes, the lazy freeze, the
  // sweep cap -- placed by hand.  A lone wave pays an issue slot for every instruction, an s_nop included, so whatever fits a
  // wait state of the rows is free and the rest is made as short as it goes:
  //   * the values at the start of the sweep are not copied: they STAY in lam / u / u2 / lam2 and the sweep works on w / wu /
  //     wu2 / w2 -- row 0 commits with a three-operand v_fma into w, `wu = u` sits in row 0's wait state, `w2 = lam2` in a
  //     wait state of the first foot pair (wu2 = u2 is the one copy that costs a slot);
  //   * the ten wait states of the foot pairs hold: the per-robot mask of the PREVIOUS sweep's votes (`live`: three
  //     instructions on the wave mask, which the previous sweep left in vcc), the body pairs' grip compare, limit and selects,
  //     the fold of the grip mask to one bit group per leg, and the first residual difference;
  //   * a leg's test is one s_and_b32 (it sets SCC) and a branch;
  //   * the residual masks are taken on the un-restored impulses and AND-ed with `live` as scalars (a restored robot's
  //     difference is 0 > tol: false -- the same votes), the AND sets SCC for the exit branch; the sweep cap counts `rem`
  //     down (s_sub_u32 borrows on the sweep that reaches the cap);
  //   * the lazy freeze is four selects on `live` at the end of the sweep.
  // 123 issue slots per sweep without a loaded body leg, 127 + 16 per loaded leg with (sweep_and_test around the three
  // blocks: 152 + 16 per leg).  Every arithmetic instruction has the operands it has there and every register sees its updates
  // in the same order: the results are the same bit for bit.  fl / fh: this lane's robot (16-lane row) in the low / high half of
  // a wave mask.  rem: K.iters - 1 on entry (at least 0); on return K.iters - 1 - (sweeps - 1), or ~0u after the cap.
  __device__ __forceinline__ void pgs_body_stream(float& lam, float& u, float& u2, float& lam2, unsigned& rem, float iA, float c0, float mue,
                                                  const float (&A)[4][3], const float* Ak, const float* mk0, const float* mk3, const float* mt,
                                                  const float* bn, const float* bt, float iA2, float body_mu, const float (&AT)[4][2],
                                                  const float (&BB)[4][2], float tol, float tol2) const {
    const unsigned row16 = 0xFFFFu << (tid & 16);
    const unsigned fl = (tid & 32) ? 0u : row16, fh = (tid & 32) ? row16 : 0u;
    float w, wu, wu2, w2, t, dA, dB, lnq, lbn, iAg, limg, lim, lc, sq, sc, iA2g, lim2g, rr;
    unsigned x, gm, tmp;
    unsigned long long live, mv, sa;
#define ETG_SGM "s_or_b32 %[gm], vcc_lo, vcc_hi\n"            /* a leg's lanes at the same bits of both halves; SCC = any  */
#define ETG_SU2(D, LP, BOP) "v_fmac_f32_dpp %[wu2], %[" D "], %[" BOP "] row_newbcast:" #LP ETG_DPPC
#define ETG_SROW(D, LP, AOP, MOP, FILL)                                              \
    "v_fma_f32 %[t], -%[wu], %[iA], %[c0]\n"                                         \
    "v_max_f32_e64 %[" D "], -%[w], %[t]\n"                                          \
    "v_fmac_f32_e32 %[w], %[" MOP "], %[" D "]\n"                                    \
    FILL                                                                             \
    "v_fmac_f32_dpp %[wu], %[" D "], %[" AOP "] row_newbcast:" #LP ETG_DPPC
#define ETG_SPAIR(D, R1, R2, A1, A2, MOP, F1, F2, F3)                                \
    "v_fma_f32 %[lc], -%[wu], %[iAg], %[w]\n"                                        \
    "v_fmaak_f32 %[sq], %[lc], %[lc], 0x0da24260\n"                                  \
    F1                                                                               \
    "v_add_f32_dpp %[sq], %[sq], %[sq] quad_perm:[0,2,1,3]" ETG_DPPC                 \
    "v_rsq_f32_e32 %[sq], %[sq]\n"                                                   \
    F2                                                                               \
    "v_mul_f32_e32 %[sc], %[limg], %[sq]\n"                                          \
    "v_min_f32_e32 %[sc], 1.0, %[sc]\n"                                              \
    "v_fma_f32 %[" D "], %[lc], %[sc], -%[w]\n"                                      \
    "v_fmac_f32_e32 %[w], %[" MOP "], %[" D "]\n"                                    \
    F3                                                                               \
    "v_fmac_f32_dpp %[wu], %[" D "], %[" A1 "] row_newbcast:" #R1 ETG_DPPC           \
    "v_fmac_f32_dpp %[wu], %[" D "], %[" A2 "] row_newbcast:" #R2 ETG_DPPC
#define ETG_SLEG(LP, LEGBITS, R1, R2, MOP)                                           \
    "s_and_b32 %[tmp], %[gm], " LEGBITS "\n"                                         \
    "s_cbranch_scc0 .Letg_sw_leg" #LP "_%=\n"                                        \
    "v_fma_f32 %[lc], -%[wu2], %[iA2g], %[w2]\n"                                     \
    "v_fmaak_f32 %[sq], %[lc], %[lc], 0x0da24260\n"                                  \
    "s_nop 1\n"                                                                      \
    "v_add_f32_dpp %[sq], %[sq], %[sq] quad_perm:[0,2,1,3]" ETG_DPPC                 \
    "v_rsq_f32_e32 %[sq], %[sq]\n"                                                   \
    "s_nop 0\n"                                                                      \
    "v_mul_f32_e32 %[sc], %[lim2g], %[sq]\n"                                         \
    "v_min_f32_e32 %[sc], 1.0, %[sc]\n"                                              \
    "v_fma_f32 %[dA], %[lc], %[sc], -%[w2]\n"                                        \
    "v_fmac_f32_e32 %[w2], %[" MOP "], %[dA]\n"                                      \
    "s_nop 0\n"                                                                      \
    "v_fmac_f32_dpp %[wu], %[dA], %[at" #LP "0] row_newbcast:" #R1 ETG_DPPC          \
    "v_fmac_f32_dpp %[wu2], %[dA], %[bb" #LP "0] row_newbcast:" #R1 ETG_DPPC         \
    "v_fmac_f32_dpp %[wu], %[dA], %[at" #LP "1] row_newbcast:" #R2 ETG_DPPC          \
    "v_fmac_f32_dpp %[wu2], %[dA], %[bb" #LP "1] row_newbcast:" #R2 ETG_DPPC         \
    ".Letg_sw_leg" #LP "_%=:\n"
    asm volatile(
        "s_mov_b64 vcc, -1\n"                                        /* votes "before the first sweep": nobody is frozen      */
        ".Letg_sw_top_%=:\n"
        /* ---- normal rows: the feet's, then the body's (pgs_normals_body2) */
        "v_mov_b32_e32 %[wu2], %[u2]\n"
        "v_fma_f32 %[t], -%[u], %[iA], %[c0]\n"
        "v_max_f32_e64 %[dA], -%[lam], %[t]\n"
        "v_fma_f32 %[w], %[m0], %[dA], %[lam]\n"                     /* row 0 commits into the working register               */
        "v_mov_b32_e32 %[wu], %[u]\n"
        "v_fmac_f32_dpp %[wu], %[dA], %[a0] row_newbcast:0" ETG_DPPC
        ETG_SROW("dB", 4, "a1", "m1", ETG_SU2("dA", 0, "b0"))
        ETG_SROW("dA", 8, "a2", "m2", ETG_SU2("dB", 4, "b1"))
        ETG_SROW("dB", 12, "a3", "m3", ETG_SU2("dA", 8, "b2"))
        ETG_SROW("dA", 3, "k0", "n0", ETG_SU2("dB", 12, "b3"))
        ETG_SROW("dB", 7, "k1", "n1", ETG_SU2("dA", 3, "b4"))
        ETG_SROW("dA", 11, "k2", "n2", ETG_SU2("dB", 7, "b5"))
        ETG_SROW("dB", 15, "k3", "n3", ETG_SU2("dA", 11, "b6"))
        ETG_SU2("dB", 15, "b7")
        /* ---- the feet's grip: friction constants of a foot without load are the identity's (pgs_tangents_disc) */
        "v_mov_b32_dpp %[lnq], %[w] quad_perm:[0,0,0,0]" ETG_DPPC
        "v_mov_b32_dpp %[lbn], %[w] quad_perm:[3,3,3,3]" ETG_DPPC
        "v_cmp_lt_f32_e64 %[sa], 0, %[lnq]\n"
        "v_mul_f32_e32 %[lim], %[mue], %[lnq]\n"
        "v_cndmask_b32_e64 %[iAg], 0, %[iA], %[sa]\n"
        "v_cndmask_b32_e64 %[limg], %[big], %[lim], %[sa]\n"
        /* ---- the feet's friction pairs (pgs_tangents_disc2); in their wait states: live, the body pairs' constants, gm, rr */
        ETG_SPAIR("dA", 1, 2, "a01", "a02", "t0",
                  "v_and_b32_e32 %[x], vcc_lo, %[fl]\n" "v_and_or_b32 %[x], vcc_hi, %[fh], %[x]\n",
                  "v_cmp_ne_u32_e64 %[live], 0, %[x]\n",
                  "v_mov_b32_e32 %[w2], %[lam2]\n")
        ETG_SPAIR("dB", 5, 6, "a11", "a12", "t1", ETG_SU2("dA", 1, "e0") ETG_SU2("dA", 2, "e1"),
                  "v_cmp_lt_f32_e32 vcc, 0, %[lbn]\n",
                  "v_mul_f32_e32 %[lim], %[bmu], %[lbn]\n")
        ETG_SPAIR("dA", 9, 10, "a21", "a22", "t2", ETG_SU2("dB", 5, "e2") ETG_SU2("dB", 6, "e3"),
                  "v_cndmask_b32_e32 %[iA2g], 0, %[iA2], vcc\n",
                  "v_cndmask_b32_e32 %[lim2g], %[big], %[lim], vcc\n")
        ETG_SPAIR("dB", 13, 14, "a31", "a32", "t3", ETG_SU2("dA", 9, "e4") ETG_SU2("dA", 10, "e5"),
                  ETG_SGM,
                  "v_sub_f32_e32 %[rr], %[w], %[lam]\n")
        ETG_SU2("dB", 13, "e6") ETG_SU2("dB", 14, "e7")
        "v_cmp_gt_f32_e64 %[mv], |%[rr]|, %[tol]\n"
        "s_cbranch_scc0 .Letg_sw_nf_%=\n"                            /* no body normal of the wave carries load               */
        /* ---- the body contacts' friction pairs (pgs_pair_body), legs without a loaded contact in the wave skipped */
        ETG_SLEG(0, "0x000f000f", 1, 2, "t0")
        ETG_SLEG(1, "0x00f000f0", 5, 6, "t1")
        ETG_SLEG(2, "0x0f000f00", 9, 10, "t2")
        ETG_SLEG(3, "0xf000f000", 13, 14, "t3")
        "v_sub_f32_e32 %[rr], %[w2], %[lam2]\n"
        "v_cmp_gt_f32_e64 %[sa], |%[rr]|, %[tol2]\n"
        "s_or_b64 %[mv], %[mv], %[sa]\n"
        "v_cndmask_b32_e64 %[lam2], %[lam2], %[w2], %[live]\n"
        ".Letg_sw_nf_%=:\n"
        /* ---- a robot that had converged before this sweep keeps its values; the votes of the others; exit tests */
        "v_cndmask_b32_e64 %[lam], %[lam], %[w], %[live]\n"
        "v_cndmask_b32_e64 %[u], %[u], %[wu], %[live]\n"
        "v_cndmask_b32_e64 %[u2], %[u2], %[wu2], %[live]\n"
        "s_and_b64 vcc, %[mv], %[live]\n"
        "s_cbranch_scc0 .Letg_sw_end_%=\n"                           /* no robot of the wave moved                            */
        "s_sub_u32 %[rem], %[rem], 1\n"
        "s_cbranch_scc0 .Letg_sw_top_%=\n"                           /* (borrow: that was sweep K.iters)                      */
        ".Letg_sw_end_%=:\n"
        : [lam] "+&v"(lam), [u] "+&v"(u), [u2] "+&v"(u2), [lam2] "+&v"(lam2), [rem] "+&s"(rem), [w] "=&v"(w), [wu] "=&v"(wu), [wu2] "=&v"(wu2),
          [w2] "=&v"(w2), [t] "=&v"(t), [dA] "=&v"(dA), [dB] "=&v"(dB), [lnq] "=&v"(lnq), [lbn] "=&v"(lbn), [iAg] "=&v"(iAg), [limg] "=&v"(limg),
          [lim] "=&v"(lim), [lc] "=&v"(lc), [sq] "=&v"(sq), [sc] "=&v"(sc), [iA2g] "=&v"(iA2g), [lim2g] "=&v"(lim2g), [rr] "=&v"(rr), [x] "=&v"(x),
          [gm] "=&s"(gm), [tmp] "=&s"(tmp), [live] "=&s"(live), [mv] "=&s"(mv), [sa] "=&s"(sa)
        : [iA] "v"(iA), [c0] "v"(c0), [mue] "v"(mue), [big] "v"(1e30f), [a0] "v"(A[0][0]), [a1] "v"(A[1][0]), [a2] "v"(A[2][0]), [a3] "v"(A[3][0]),
          [m0] "v"(mk0[0]), [m1] "v"(mk0[1]), [m2] "v"(mk0[2]), [m3] "v"(mk0[3]),
          [k0] "v"(Ak[0]), [k1] "v"(Ak[1]), [k2] "v"(Ak[2]), [k3] "v"(Ak[3]),
          [n0] "v"(mk3[0]), [n1] "v"(mk3[1]), [n2] "v"(mk3[2]), [n3] "v"(mk3[3]),
          [b0] "v"(bn[0]), [b1] "v"(bn[1]), [b2] "v"(bn[2]), [b3] "v"(bn[3]), [b4] "v"(bn[4]), [b5] "v"(bn[5]), [b6] "v"(bn[6]), [b7] "v"(bn[7]),
          [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a11] "v"(A[1][1]), [a12] "v"(A[1][2]), [a21] "v"(A[2][1]), [a22] "v"(A[2][2]),
          [a31] "v"(A[3][1]), [a32] "v"(A[3][2]), [t0] "v"(mt[0]), [t1] "v"(mt[1]), [t2] "v"(mt[2]), [t3] "v"(mt[3]),
          [e0] "v"(bt[0]), [e1] "v"(bt[1]), [e2] "v"(bt[2]), [e3] "v"(bt[3]), [e4] "v"(bt[4]), [e5] "v"(bt[5]), [e6] "v"(bt[6]), [e7] "v"(bt[7]),
          [iA2] "v"(iA2), [bmu] "s"(body_mu), [at00] "v"(AT[0][0]), [at01] "v"(AT[0][1]), [at10] "v"(AT[1][0]), [at11] "v"(AT[1][1]),
          [at20] "v"(AT[2][0]), [at21] "v"(AT[2][1]), [at30] "v"(AT[3][0]), [at31] "v"(AT[3][1]),
          [bb00] "v"(BB[0][0]), [bb01] "v"(BB[0][1]), [bb10] "v"(BB[1][0]), [bb11] "v"(BB[1][1]),
          [bb20] "v"(BB[2][0]), [bb21] "v"(BB[2][1]), [bb30] "v"(BB[3][0]), [bb31] "v"(BB[3][1]),
          [tol] "v"(tol), [tol2] "v"(tol2), [fl] "v"(fl), [fh] "v"(fh)
        : "vcc", "scc");
#undef ETG_SGM
#undef ETG_SU2
#undef ETG_SROW
#undef ETG_SPAIR
#undef ETG_SLEG
  }
#endif
#undef ETG_DPPC
  // every value that later feeds fmac_rbcast / fmac_qb as the broadcast source passes through here: the
  // asm "modifies" them, so their producers are ordered before it and the DPP reads after it
  __device__ __forceinline__ void dpp_ready10(float* z, float* hj, float* lam) const {
    asm volatile("s_nop 1" : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]), "+v"(hj[0]), "+v"(hj[1]), "+v"(hj[2]), "+v"(lam[0]));
  }
  // 32 floats of per-lane scratch in the lane's LDS parameter column: the fields that the 16-lane kernels never stage
  // (kStaged16 below: the link block PR_LINK..PR_LINK+29 and the gains go straight to registers through tpar*)
  __device__ __forceinline__ static int slotb_field(int k) { return k < 30 ? PR_LINK + k : PR_KP + (k - 30); }
  __device__ __forceinline__ void slotb_st(int k, float v) const { const_cast<float*>(lds)[slotb_field(k) * 64] = v; }
  __device__ __forceinline__ float slotb_ld(int k) const { return lds[slotb_field(k) * 64]; }
  // an optimisation barrier without an instruction: the value's producer cannot be fused into its consumers (etg_core16.h)
  __device__ __forceinline__ void opaque(float& v) const { asm volatile("" : "+v"(v)); }
  __device__ __forceinline__ void opaque3(float* v) const { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2])); }
  __device__ __forceinline__ void dpp_ready(float* v, int n) const {
    if (n == 6) asm volatile("s_nop 1" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
    else if (n == 3) asm volatile("s_nop 1" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
    else asm volatile("s_nop 1" : "+v"(v[0]));
  }
  // ---- memory (same SoA arrays as the 4-lane kernels)
  __device__ __forceinline__ float ld_joint(const float* p, int f0) const { return p[(size_t)(f0 + sc) * NL + col]; }
  __device__ __forceinline__ void st_joint(float* p, int f0, float v) const { if (gate && sub < 3) p[(size_t)(f0 + sub) * NL + col] = v; }
  // four fields f0 .. f0 + 3, one per lane of the leg (LG_LAM .. LG_LAMB: the foot's three impulses and the body contact's normal)
  __device__ __forceinline__ float ld_quad(const float* p, int f0) const { return p[(size_t)(f0 + sub) * NL + col]; }
  __device__ __forceinline__ void st_quad(float* p, int f0, float v) const { if (gate) p[(size_t)(f0 + sub) * NL + col] = v; }
  __device__ __forceinline__ float ld_legf(const float* p, int f) const { return p[(size_t)f * NL + col]; }
  __device__ __forceinline__ void st_legf(float* p, int f, float v) const { if (gate && sub == 0) p[(size_t)f * NL + col] = v; }
  __device__ __forceinline__ float ld_env(const float* p, int f) const { return p[(size_t)f * N + env]; }
  // field f0 + stride * sub of the per-robot array: the 4 sub-lanes of a leg split a table between them
  __device__ __forceinline__ float ld_env_sub(const float* p, int f0, int stride) const { return p[(size_t)(f0 + stride * sub) * N + env]; }
  __device__ __forceinline__ void st_env(float* p, int f, float v) const { if (gate && r == 0) p[(size_t)f * N + env] = v; }
  __device__ __forceinline__ int ld_env_i(const int* p, int f) const { return p[(size_t)f * N + env]; }
  __device__ __forceinline__ void st_env_i(int* p, int f, int v) const { if (gate && r == 0) p[(size_t)f * N + env] = v; }
  __device__ __forceinline__ void st_ring_joint(float* rg, int slot, int k0, float v) const { if (gate && sub < 3) rg[((size_t)slot * 8 + k0 + sub) * NL + col] = v; }
  __device__ __forceinline__ void st_ring_aux(float* rg, int slot, int k, float v) const { if (gate && sub == 3) rg[((size_t)slot * 8 + k) * NL + col] = v; }
  __device__ __forceinline__ float ld_ring_joint(const float* rg, int slot, int k0) const { return rg[((size_t)slot * 8 + k0 + sc) * NL + col]; }
  __device__ __forceinline__ float ld_ring_k(const float* rg, int slot, int k) const { return rg[((size_t)slot * 8 + k) * NL + col]; }
  __device__ __forceinline__ float ld_row_joint(const float* p, int rowlen, int col0) const { return sub < 3 ? p[(size_t)(env - row_base) * rowlen + col0 + 3 * leg + sub] : 0.0f; }
  // element k of this lane's motor in rows of `stride` values per motor (HYBRID commands: stride 5)
  __device__ __forceinline__ float ld_row_motor(const float* p, int rowlen, int stride, int k) const { return sub < 3 ? p[(size_t)(env - row_base) * rowlen + stride * (3 * leg + sub) + k] : 0.0f; }
  __device__ __forceinline__ void st_row_joint(float* p, int rowlen, int col0, float v) const { if (gate && sub < 3) p[(size_t)(env - row_base) * rowlen + col0 + 3 * leg + sub] = v; }
  __device__ __forceinline__ void st_row_leg(float* p, int rowlen, int col0, float v) const { if (gate && sub == 0) p[(size_t)(env - row_base) * rowlen + col0 + leg] = v; }
  __device__ __forceinline__ void st_row_env(float* p, int rowlen, int c_, float v) const { if (gate && r == 0) p[(size_t)(env - row_base) * rowlen + c_] = v; }
  __device__ __forceinline__ float ld_row_env(const float* p, int rowlen, int c_) const { return p[(size_t)(env - row_base) * rowlen + c_]; }
  // phase boundary of the 16-lane tick: no scheduling barrier in the product build.  A barrier here makes the tail of one
  // phase's dependent chain (the LDL^T solve, a DPP reduction) sit out its latency before the next phase may start; without
  // it the scheduler overlaps the two, registers and scratch stay where they were, and the headline rollout runs 3-6 %
  // faster (profiles/r07_ab_experiments.txt section 5).  The profiling build keeps them around its s_memtime stamps so
  // that every stamp closes exactly its own phase.
  __device__ __forceinline__ void phase([[maybe_unused]] int id) const {
#ifdef ETG_PROFILE_PHASES
    __builtin_amdgcn_sched_barrier(0);
    long long t = clock64();
    prof[id] += t - prof_last;
    prof_last = t;
    __builtin_amdgcn_sched_barrier(0);
#endif
  }
  // a marker that exists in the profiling build only (no scheduling barrier in the product build)
  __device__ __forceinline__ void phase_p([[maybe_unused]] int id) const {
#ifdef ETG_PROFILE_PHASES
    phase(id);
#endif
  }
#ifdef ETG_PROFILE_PHASES
  mutable long long prof[16];
  mutable long long prof_last;
#endif
  __device__ __forceinline__ void terrain(const KCfg& K, float x, float y, float& h, float& nx, float& ny, float& nz) const {
    if (K.terrain == 0) { h = 0.0f; nx = 0.0f; ny = 0.0f; nz = 1.0f; }
    else heightfield_query(K, env, x, y, h, nx, ny, nz);
  }
  __device__ __forceinline__ void terrain_fetch(const KCfg& K, float x, float y, float* tap) const { heightfield_fetch(K, env, x, y, tap); }
  __device__ __forceinline__ void terrain_finish(const KCfg& K, const float* tap, float& h, float& nx, float& ny, float& nz) const {
    heightfield_finish(K, tap, h, nx, ny, nz);
  }
};
// KNEE: the body contacts of EtgConfig.body_contacts 1 / 2 (etg_core16.h) are compiled in; SLOTB_LDS: see kSlotBLds.
// PLAIN: the default robot layer -- POSITION control, no action filter / interpolation, no torque limit, no command
// clip, no external force (plain_config) -- with those options compiled out: their never-taken branches and the
// registers they pin cost the step kernels ~3 % (measured A/B), so the common configuration gets its own instantiation.
template <bool FLAT, bool KNEE = false, bool PLAIN = false, bool SLOTB_LDS = false> struct GpuCtx16T : GpuCtx16 {
  static constexpr bool kFlat = FLAT;
  static constexpr bool kKnee = KNEE;
  static constexpr bool kPlain = PLAIN;
  static constexpr bool kSlotBLds = SLOTB_LDS;   // the body friction rows' Delassus columns live in LDS (etg_core16.h: finish_tick)
  static constexpr bool kStepLocal = false;      // (GpuCtx16W: rollout constants are formed anew every control step)
#ifdef ETG_NO_ASM_SWEEP
  static constexpr bool kAsmSweep = false;
#else
  static constexpr bool kAsmSweep = true;     // pgs_normals / pgs_tangents_disc: the hand-scheduled sweep
#endif
  // the Delassus columns A / Ak and the body friction rows' BA come from the matrix pipe, four columns per instruction
  // (gram16.h); -DETG_GRAM_DPP (A/B build variant): the broadcast-FMA form, which is also the C++ statement of the columns
#ifdef ETG_GRAM_DPP
  static constexpr bool kGramMfma = false;
#else
  static constexpr bool kGramMfma = true;
#endif
  // (the round-7 form, sweep_and_test's own statements around the asm blocks, measured against it: profiles/r08_ab_experiments.txt)
#ifdef ETG_NO_ASM_SWEEP
  static constexpr bool kSweepStream = false;
#else
  static constexpr bool kSweepStream = true;  // pgs_body_stream: the body tail's residual-rule loop, bookkeeping included
#endif
};

// The context of the per-wave closed-loop kernels: the tick constants come from the lane's LDS column (staged in full at kernel
// start) instead of HBM, so that control_step can re-read them at the top of every control step -- they need not stay in
// registers across the policy tile (45 registers per lane that the allocator otherwise spills to scratch around the tile).
template <bool FLAT, bool KNEE, bool PLAIN> struct GpuCtx16W : GpuCtx16T<FLAT, KNEE, PLAIN> {
  static constexpr bool kStepLocal = true;
  __device__ __forceinline__ float tpar(int k) const { return this->lds[k * 64]; }
  __device__ __forceinline__ float tpar_joint(int base) const { return this->lds[(base + this->sc) * 64]; }
  __device__ __forceinline__ float tpar_link(int k) const { return this->sub < 3 ? this->lds[(PR_LINK + 10 * this->sub + k) * 64] : 0.0f; }
};
// register parking around the policy tile: the robot state and the control variables of the lane, in LDS (one column per lane)
constexpr int PARK16 = 36;
__device__ __forceinline__ void park16(float* p, const State16<float>& L, const StepCtl16<float>& S) {
  const float v[PARK16] = {L.p.x, L.p.y, L.p.z, L.qx, L.qy, L.qz, L.qw, L.wb.x, L.wb.y, L.wb.z, L.vb.x, L.vb.y, L.vb.z, L.q, L.qd, L.lam, L.contact,
                           __int_as_float(S.step_count), __int_as_float(S.tick), __int_as_float(S.has_last), S.last, S.lbx, S.lby, S.lbz, S.last_fwx,
                           S.ret, S.len, S.r0, S.r1, S.r2, S.fx0, S.fx1, S.fy0, S.fy1, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < PARK16; k++) p[k * 64] = v[k];
}
__device__ __forceinline__ void unpark16(const float* p, State16<float>& L, StepCtl16<float>& S) {
  float v[PARK16];
#pragma unroll
  for (int k = 0; k < PARK16; k++) v[k] = p[k * 64];
  L.p = {v[0], v[1], v[2]}; L.qx = v[3]; L.qy = v[4]; L.qz = v[5]; L.qw = v[6];
  L.wb = {v[7], v[8], v[9]}; L.vb = {v[10], v[11], v[12]}; L.q = v[13]; L.qd = v[14]; L.lam = v[15]; L.contact = v[16];
  S.step_count = __float_as_int(v[17]); S.tick = __float_as_int(v[18]); S.has_last = __float_as_int(v[19]);
  S.last = v[20]; S.lbx = v[21]; S.lby = v[22]; S.lbz = v[23]; S.last_fwx = v[24]; S.ret = v[25]; S.len = v[26];
  S.r0 = v[27]; S.r1 = v[28]; S.r2 = v[29]; S.fx0 = v[30]; S.fx1 = v[31]; S.fy0 = v[32]; S.fy1 = v[33];
}

// robot_block = index of the group of 4 robots this wave carries, lane = lane in the wave, lds_wave = the wave's
// own [LDS16_FIELDS][64] parameter staging area.  Three steps so that a caller can put its own loads between the staging
// loads and the LDS writes that have to wait for them (step16_body: one HBM round trip at the head of the launch, not two).
constexpr int kStaged16[] = {PR_O1, PR_O1 + 1, PR_O1 + 2, PR_SY, PR_LAT_N, PR_LAT_A, PR_BASE_FOOT, PR_BASE_FOOT + 1,
                             PR_BASE_FOOT + 2, PR_POSE, PR_POSE + 1, PR_POSE + 2, PR_EMEAN, PR_EMEAN + 1, PR_EMEAN + 2,
                             PR_ESTD, PR_ESTD + 1, PR_ESTD + 2, PR_HIPSIGN};
constexpr int kNStaged16 = sizeof(kStaged16) / sizeof(int);
__device__ __forceinline__ bool make_ctx16_fields(const KCfg& K, const DevState& D, GpuCtx16& c, float* lds_wave, int robot_block, int lane) {
  c.tid = lane;
  c.env = robot_block * 4 + (lane >> 4);
  c.r = lane & 15;
  c.leg = c.r >> 2;
  c.sub = c.r & 3;
  c.sc = c.sub < 2 ? c.sub : 2;
  c.N = K.n_env;
  c.NL = 4 * K.n_env;
  if (c.env >= c.N) return false;   // whole rows drop out together, so every DPP/MFMA group stays complete
  c.col = (size_t)4 * c.env + c.leg;
  c.gpar = D.par;
  c.lds = lds_wave + lane;
  return true;
}
// stage in LDS only the leg-level parameters that the once-per-step code reads (c.par / c.par_joint); the tick
// constants (gains, link block, gravity, trunk inertia, mu) go straight to registers through tpar*
__device__ __forceinline__ void stage16_issue(const DevState& D, const GpuCtx16& c, float (&v)[kNStaged16]) {
#pragma unroll
  for (int i = 0; i < kNStaged16; i++) v[i] = D.par[(size_t)kStaged16[i] * c.NL + c.col];
}
__device__ __forceinline__ void stage16_commit(const GpuCtx16& c, const float (&v)[kNStaged16]) {
  float* mine = const_cast<float*>(c.lds);
#pragma unroll
  for (int i = 0; i < kNStaged16; i++) mine[kStaged16[i] * 64] = v[i];
}
__device__ __forceinline__ bool make_ctx16_at(const KCfg& K, const DevState& D, GpuCtx16& c, float* lds_wave, int robot_block, int lane) {
  if (!make_ctx16_fields(K, D, c, lds_wave, robot_block, lane)) return false;
  float v[kNStaged16];
  stage16_issue(D, c, v);
  stage16_commit(c, v);
  return true;
}
__device__ __forceinline__ bool make_ctx16(const KCfg& K, const DevState& D, GpuCtx16& c, float* lds_all) {
  return make_ctx16_at(K, D, c, lds_all, xcd_contiguous_block(), threadIdx.x);
}

template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_settle16(KCfg K, DevState D, const uint8_t* mask) {
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];
  GpuCtx16T<FLAT, KNEE, PLAIN> c;
  if (!make_ctx16(K, D, c, lds_par)) return;
  if ((mask && !mask[c.env]) || settle_cached<FLAT>(K, D, c.env)) return;   // whole rows drop out together
  State16<float> L;
  const float ox = D.reset_off[c.env], oy = D.reset_off[K.n_env + c.env];
  reset_settle16(c, K, L, D.ring, ox, oy);
  store_state16(c, D.cache_base, D.cache_leg, L);
  store_state16(c, D.base, D.leg, L);
  settle_mark_fresh(K, D, c.env, ox, oy);
}

// reset_finish16 from the cache: same stores, no arithmetic
template <class Ctx>
__device__ __forceinline__ void restart_from_cache16(const Ctx& c, const KCfg& K, State16<float>& L, float* ctl, int* ictl, float* legctl,
                                                     const float* fin, float* obs) {
  const int N = K.n_env;
  const float pose = c.jointf() * c.par_joint(PR_POSE);
  L.energy = 0.0f;
  c.st_env_i(ictl, IC_STEP, 0);
  c.st_env_i(ictl, IC_TICK, K.settle_ticks);
  c.st_env_i(ictl, IC_HAS_LAST, 0);
  c.st_env(ctl, CT_RET, 0.0f); c.st_env(ctl, CT_LEN, 0.0f); c.st_env(ctl, CT_ALIVE, 1.0f);
  c.st_env(ctl, CT_LAST_BASE + 0, L.p.x); c.st_env(ctl, CT_LAST_BASE + 1, L.p.y); c.st_env(ctl, CT_LAST_BASE + 2, L.p.z);
  c.st_joint(legctl, LC_LAST_QDES, pose);
  c.st_joint(legctl, LC_FX0, pose); c.st_joint(legctl, LC_FX1, pose);
  c.st_joint(legctl, LC_FY0, pose); c.st_joint(legctl, LC_FY1, pose);
  c.st_legf(legctl, LC_LAST_FOOT_X, fin[(size_t)(FIN_FWX + c.leg) * N + c.env]);
#pragma unroll
  for (int k = 0; k < 3; k++) c.st_env(ctl, CT_FIRST_RPY + k, fin[(size_t)(FIN_RPY + k) * N + c.env]);
  for (int k = c.r; k < ETG_OBS_DIM; k += 16) obs[(size_t)(c.env - c.row_base) * ETG_OBS_DIM + k] = fin[(size_t)(FIN_OBS + k) * N + c.env];
}

template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_finish16(KCfg K, DevState D, const uint8_t* mask, float* obs) {
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];
  GpuCtx16T<FLAT, KNEE, PLAIN> c;
  if (!make_ctx16(K, D, c, lds_par)) return;
  if (mask && !mask[c.env]) return;
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  reset_finish16(c, K, L, D.ring, D.ctl, D.ictl, D.legctl, D.etgp, obs);
  store_state16(c, D.base, D.leg, L);
}

// The restart of a robot whose step ended its episode, inside the step's launch (every robot has a cached settle): prepared
// next-episode parameters installed (NX), cached settle -> registers, reset_finish (control state, episode accumulators, first
// observation over the robot's row of `obs`; the pre-reset ring readings come from KCfg.cring), pending push cleared.  Called
// by whole 16-lane rows (a robot's lanes together): step16_body<AUTO> and step_policy16_body<AUTO>.
template <class Ctx>
__device__ __forceinline__ void restart16(const Ctx& c, const KCfg& K, const DevState& D, const NextDyn& NX, State16<float>& L, float* obs) {
  const int N = K.n_env;
  if (NX.ok && NX.ok[c.env]) {   // parameters prepared for the next episode: install them (the cached settle below is theirs)
    for (int k = c.sub; k < PR_DERIVED; k += 4) D.par[(size_t)k * c.NL + c.col] = NX.par[(size_t)k * c.NL + c.col];   // a leg's 4 lanes share its column
    for (int k = c.r; k < ETG_DYN_DIM; k += 16) D.dyn[(size_t)c.env * ETG_DYN_DIM + k] = NX.dyn[(size_t)c.env * ETG_DYN_DIM + k];
    __builtin_amdgcn_s_waitcnt(0);          // the row's reads of the flag and its stores are done before lane 0 clears it
    __builtin_amdgcn_wave_barrier();
    if (c.r == 0) NX.ok[c.env] = 0;
    float stg2[kNStaged16];                 // the restart below reads the staged leg parameters: the new ones
    stage16_issue(D, c, stg2);
    stage16_commit(c, stg2);
  }
  L = load_state16<float>(c, D.cache_base, D.cache_leg);
  L.p.x += D.reset_off[c.env] - D.cache_off[c.env];        // non-zero only on flat ground (settle_cached)
  L.p.y += D.reset_off[N + c.env] - D.cache_off[N + c.env];
  if (D.cache_off[(size_t)FIN_OK * N + c.env] > 0.5f) restart_from_cache16(c, K, L, D.ctl, D.ictl, D.legctl, D.cache_off, obs);
  else reset_finish16(c, K, L, D.ring, D.ctl, D.ictl, D.legctl, D.etgp, obs);
  if (c.r == 0) {
    D.ictl[(size_t)IC_PUSH_LEFT * N + c.env] = 0;
    for (int k = 0; k < 3; k++) D.ctl[(size_t)(CT_PUSH + k) * N + c.env] = 0.0f;
  }
}

// env.step for the 4 robots of a wave.  AUTO (etg_step_autoreset while every robot has a cached settle): a robot whose step
// ended its episode restarts inside the same launch (restart16), its first observation over the step's row.  reward / done /
// info stay the finished step's.  T (AUTO only, etg_step_autoreset_terminal): the step's row of every robot also goes to T.obs,
// and a restarting robot's pre-restart sensor context to T.ctx.
template <bool FLAT, bool KNEE, bool PLAIN, bool AUTO>
__device__ __forceinline__ void step16_body(const KCfg& K, const DevState& D, const float* action, const uint8_t* donef, float* obs,
                                            float* reward, uint8_t* done, float* info, float* lds_par, const NextDyn NX = NextDyn{nullptr, nullptr, nullptr},
                                            const TermOut T = TermOut{nullptr, nullptr}) {
  GpuCtx16T<FLAT, KNEE, PLAIN> c;
  if (!make_ctx16_fields(K, D, c, lds_par, K.block0 + xcd_contiguous_block(), threadIdx.x)) return;   // (block0: etg_step_range)
  // the head of a launch is a chain of cold loads (the L2s are invalidated at kernel boundaries): ALL of them -- staged
  // parameters, state, control state, tick constants, action, done flag -- are requested before the first use, so the launch
  // pays one HBM round trip here instead of one per group (the LDS writes of the staging used to wait in front of the rest)
  float stg[kNStaged16];
  stage16_issue(D, c, stg);
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  StepCtl16<float> S = load_ctl16<float>(c, K, D.ctl, D.ictl, D.legctl);
  TickPar<float> tp = load_tick_par<float>(c);
  if (!PLAIN && K.ext_force) tp.fext = load_fext16<float>(c, D.ctl);
  const bool hybrid = K.motor_mode == 2 && action;   // rows of 60: per motor (q_des, kp, qd_des, kd, tau_ff)
  float act = !action ? 0.0f : hybrid ? c.ld_row_motor(action, ETG_HYBRID_DIM, 5, 0) : c.ld_row_joint(action, ETG_ACT_DIM, 0);
  float hyb[4];
#pragma unroll
  for (int k = 0; k < 4; k++) hyb[k] = hybrid ? c.ld_row_motor(action, ETG_HYBRID_DIM, 5, 1 + k) : 0.0f;
  const float dflag = donef ? (float)donef[c.env] : 0.0f;
  stage16_commit(c, stg);
  float r, d;
#ifdef ETG_PROFILE_PHASES
  for (int k = 0; k < 16; k++) c.prof[k] = 0;
  c.prof_last = clock64();
  long long t_begin = c.prof_last;
#endif
  control_step16_core(c, K, tp, L, S, D.ring, D.etgp, act, dflag, obs, r, d, info, hybrid ? hyb : nullptr, true, nullptr, nullptr,
                      false, nullptr, AUTO ? T.obs : (float*)nullptr);
  store_ctl16(c, K, S, D.ctl, D.ictl, D.legctl);
  if (AUTO && d > 0.5f) {   // whole 16-lane rows take this branch together (d is the robot's)
    if (T.ctx) term_ctx_store(K, D, c.env, c.r, 16, S.step_count, T.ctx);
    restart16(c, K, D, NX, L, obs);
  }
  store_state16(c, D.base, D.leg, L);
#ifdef ETG_PROFILE_PHASES
  if ((c.env & 3) == 0 && c.r == 0 && info) {   // every wave reports, in the info row of its first robot
    float* row = info + (size_t)c.env * ETG_INFO_DIM;
    for (int k = 0; k < 16; k++) row[k] = (float)c.prof[k];
    row[16] = (float)(clock64() - t_begin);
  }
#endif
  if (c.r == 0) {
    reward[c.env] = r;
    done[c.env] = d > 0.5f ? 1 : 0;
  }
}
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_step16(KCfg K, DevState D, const float* action, const uint8_t* donef, float* obs,
                                                   float* reward, uint8_t* done, float* info) {
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];
  step16_body<FLAT, KNEE, PLAIN, false>(K, D, action, donef, obs, reward, done, info, lds_par);
}
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_step16_ar(KCfg K, DevState D, const float* action, const uint8_t* donef, float* obs,
                                                      float* reward, uint8_t* done, float* info, NextDyn NX, TermOut T) {
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];
  step16_body<FLAT, KNEE, PLAIN, true>(K, D, action, donef, obs, reward, done, info, lds_par, NX, T);
}

// n_steps open-loop control steps of every robot in one launch (rollout_steps16): state, control variables and
// tick constants stay in registers between the steps
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_rollout16(KCfg K, DevState D, int n_steps, float* obs, StatOut so) {
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];
  // rollout constants hoisted to the kernel's head, tick constants from HBM.  (Formed anew every control step like the tape and
  // closed-loop kernels: 343 registers instead of 448 and 60 % fewer accumulator-register moves, and 0.4 % SLOWER on the same
  // box: profiles/r06_ab_experiments.txt section 5)
  GpuCtx16T<FLAT, KNEE, PLAIN> c;
  if (!make_ctx16(K, D, c, lds_par)) return;
  const long long t0 = so.cyc ? clock64() : 0;
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  rollout_steps16(c, K, L, D.base, D.leg, D.ring, D.ctl, D.ictl, D.legctl, D.etgp, n_steps, obs);   // (stores the state itself: stop_at_done)
  if (so.cyc && threadIdx.x == 0) so.cyc[blockIdx.x] = clock64() - t0;
  if (so.ret && c.r == 0) {   // the last launch of a rollout hands the episode statistics to the caller itself (no extra launch):
    so.ret[c.env] = D.ctl[(size_t)CT_RET * K.n_env + c.env];        // lane 0 of the robot's row re-reads what it has just stored
    so.len[c.env] = (int)D.ctl[(size_t)CT_LEN * K.n_env + c.env];
  }
}

// the 16-lane counterpart of k_rollout_actions
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_rollout_actions16(KCfg K, DevState D, int n_steps, const float* actions, float* obs, TapeOut T) {
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];
  GpuCtx16W<FLAT, KNEE, PLAIN> c;             // (rollout constants formed anew every control step: see rollout_steps16)
  if (!make_ctx16_fields(K, D, c, lds_par, xcd_contiguous_block(), threadIdx.x)) return;
  for (int k = 0; k < PR_N; k++) lds_par[k * 64 + threadIdx.x] = D.par[(size_t)k * c.NL + c.col];
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  StepCtl16<float> S = load_ctl16<float>(c, K, D.ctl, D.ictl, D.legctl);
  V3<float> fext = {0.0f, 0.0f, 0.0f};
  if (!PLAIN && K.ext_force) fext = load_fext16<float>(c, D.ctl);
  const size_t N = K.n_env;
  float reward, done;
  const bool skip = K.stop_at_done != 0;
  for (int s = 0; s < n_steps; s++) {
    c.launder_lane();
    TickPar<float> tp = load_tick_par<float>(c);
    tp.fext = fext;
    const float act = c.ld_row_joint(actions + (size_t)s * N * ETG_ACT_DIM, ETG_ACT_DIM, 0);
    const bool last = s == n_steps - 1;
    const float was_alive = S.alive;
    if (!skip || c.any(was_alive > 0.5f)) {   // (see k_rollout_actions)
      control_step16_core(c, K, tp, L, S, D.ring, D.etgp, act, 0.0f, (T.obs && !last) ? T.obs + (size_t)s * N * ETG_OBS_DIM : obs, reward, done,
                          (float*)nullptr, (const float*)nullptr, last || T.obs || T.imu, T.q ? T.q + (size_t)s * N * ETG_ACT_DIM : nullptr,
                          T.imu ? T.imu + (size_t)s * N * 6 : nullptr, skip, obs);
      if (skip) rollout_dead_store16(c, K, L, was_alive, done, last, true, (int)K.noise_call + s, D.base, D.leg, D.ictl);
    } else {
      reward = 0.0f; done = 1.0f;
    }
    if (c.r == 0) {
      if (T.rew) T.rew[(size_t)s * N + c.env] = reward;
      if (T.done) T.done[(size_t)s * N + c.env] = done > 0.5f ? 1 : 0;
    }
  }
  store_ctl16(c, K, S, D.ctl, D.ictl, D.legctl);
  rollout_store16(c, K, L, S.alive, D.base, D.leg);
}

// Closed-loop rollout in one launch: a workgroup of 4 waves owns 16 robots = one 16-row tile of the policy MLP
// (policy_core.h).  Per control step: observations of the 16 robots (LDS) -> policy on MFMA (the 4 waves share
// the tile like k_policy) -> tanh(mean) * act_scale in LDS -> every wave runs its 4 robots' control step, writing
// the next observation back to LDS.  Nothing but the final observation, the ring and the episode accumulators
// touches HBM between steps.  (run_EStrain_episode / run_evaluate_episodes, train.py:182-249, with a fixed actor.)
struct PolicyW { const float4 *w1, *w2, *w3; const float *b1, *b2, *b3; int in_dim, out_dim, col0; };   // col0: first observation column the actor sees
// (the per-wave kernels: w1 = the k_pack_wave12 stream of both hidden layers, w2 unused, w3 / RecOut::w3s = the k_pack_head copies)
// per-step outputs of the recording variant ([n_steps][N][...]); noise != NULL: the STOCHASTIC actor of SAC.sample
// (alg/sac.py:65-76) on the caller's N(0,1) draws [n_steps][N][12]: x = mean + exp(clamp(log_std, -20, 2)) * noise,
// action = tanh(x); w3s / b3s = the packed log-std head (etg_policy_load_std)
struct RecOut { float *obs, *act, *rew; uint8_t* done; const float* noise; const float4* w3s; const float* b3s; };

// ONE body for the closed-loop kernel and its recording variant (REC: every step's observation, unscaled action, reward and done
// written out for the replay memory of the ES-SAC loop, run_EStrain_episode with es_rpm, train.py:213-249).  Two __global__
// symbols instantiate it: REC is a compile-time constant in each, so the plain kernel contains none of the recording code (a
// runtime flag in ONE kernel shifts its 512-register allocation; round 2 kept a 70-line copy for that reason, which let fixes
// diverge).  ps_mem: the [NWP][TM][16] partial sums of the log-std head (REC only).
// BF16: both kernels pass true -- precision 0 runs the per-wave kernels, so the fp32 tile has no caller and is not instantiated.
// Its side of the body (the rings started one stage early, policy_core.h: ring_prefetch / head_prefetch) stays as text:
// without it the compiler orders the instructions of all 12 bf16 tile kernels differently (same registers, same scratch), and
// these kernels sit at the 512-register limit -- profiles/dead_paths_isa_identity.txt has the comparison.
template <bool FLAT, bool BF16, bool KNEE, bool PLAIN, bool REC>
__device__ __forceinline__ void rollout_policy16_body(const KCfg& K, const DevState& D, const PolicyW& P, int n_steps, float act_scale,
                                                      float* obs, const RecOut& R, float* bufA, float* bufB, float (*part)[pol::TM][16],
                                                      float (*part_s)[pol::TM][16], float (*act_lds)[16], float* obs_lds, float* lds_par, float* live_lds) {
  using namespace pol;
  constexpr int NWP = 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = xcd_contiguous_block();            // 16 robots; the host guarantees N % 16 == 0
  GpuCtx16T<FLAT, KNEE, PLAIN, true> c;
  make_ctx16_at(K, D, c, lds_par + wave * (LDS16_FIELDS * 64), 4 * tile + wave, lane);
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  StepCtl16<float> S = load_ctl16<float>(c, K, D.ctl, D.ictl, D.legctl);
  TickPar<float> tp = load_tick_par<float>(c);
  if (!PLAIN && K.ext_force) tp.fext = load_fext16<float>(c, D.ctl);
  // current observation of the tile -> LDS
  for (int idx = tid; idx < TM * ETG_OBS_DIM; idx += 256) obs_lds[idx] = obs[(size_t)tile * TM * ETG_OBS_DIM + idx];
  float reward, done;
  // KCfg.stop_at_done: a finished robot is not simulated any more (control_step16_core).  Its row of the observation tile stays
  // its last one (the policy keeps evaluating it: a workgroup's 16 rows are one MFMA tile either way); a wave whose four robots
  // have all finished skips its control steps, a workgroup whose sixteen have leaves the loop.
  const bool skip = K.stop_at_done != 0;
  if (lane < 4) live_lds[4 * wave + lane] = 1.0f;
#ifdef ETG_PROFILE_PHASES
  long long pp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pl = clock64();
#endif
  int s_at = 0;   // the step the loop stands at (== n_steps unless the workgroup left early)
  for (int s = 0; s < n_steps; s++, s_at = s) {
    if (skip) {
      if (!__syncthreads_or(S.alive > 0.5f)) break;   // (the barrier of the loop top, with the vote riding on it)
    } else {
      __syncthreads();
    }
    if (K.noise_on && s > 0) {   // sensor noise on the row the previous step left in LDS (the last one: the launch's epilogue)
      if (live_lds[tid >> 4] > 0.5f)   // ... if the step wrote one: a robot that had finished before it keeps its row as it is
        add_sensor_noise(K, tile * TM + (tid >> 4), K.noise_call + s - 1, tid & 15, &obs_lds[(tid >> 4) * ETG_OBS_DIM]);
      __syncthreads();
    }
    // fp32: every layer's first weight fragments are requested one stage EARLY (layer 1's before the observation tile is
    // staged, layer 2's before layer 1's MFMAs, the head's before layer 2's): a lone wave per SIMD has nothing else to hide
    // the L2 latency of a layer's first fragments behind
    WRing<4, NWP> ring1;
    WRing<HID / 16, NWP> ring2;
    HeadFrag<NWP> head;
    constexpr bool PRE = !BF16;
    if (PRE) ring_prefetch(ring1, P.w1, wave, lane);
    for (int idx = tid; idx < TM * 64; idx += 256) {   // obs tile, zero padded to the 64-wide K of layer 1
      const int r = idx >> 6, col = idx & 63;
      bufA[r * HS + col] = col < P.in_dim ? obs_lds[r * ETG_OBS_DIM + P.col0 + col] : 0.0f;
    }
    if (REC)   // the observation the actor acts on at this step (noise included), rows of the tile's 16 robots: coalesced
      for (int idx = tid; idx < TM * ETG_OBS_DIM; idx += 256) R.obs[((size_t)s * K.n_env + (size_t)tile * TM) * ETG_OBS_DIM + idx] = obs_lds[idx];
    __syncthreads();
#ifdef ETG_PROFILE_PHASES
    { long long t = clock64(); pp[0] += t - pl; pl = t; __builtin_amdgcn_sched_barrier(0); }
#endif
    if (PRE) ring_prefetch(ring2, P.w2, wave, lane);
    hidden_layer<BF16, 4, NWP, PRE>(bufA, P.w1, P.b1, bufB, wave, lane, &ring1);
    __syncthreads();
#ifdef ETG_PROFILE_PHASES
    { long long t = clock64(); pp[1] += t - pl; pl = t; __builtin_amdgcn_sched_barrier(0); }
#endif
    if (PRE) head_prefetch(head, P.w3, wave, lane);
    hidden_layer<BF16, HID / 16, NWP, PRE>(bufB, P.w2, P.b2, bufA, wave, lane, &ring2);
    __syncthreads();
#ifdef ETG_PROFILE_PHASES
    { long long t = clock64(); pp[2] += t - pl; pl = t; __builtin_amdgcn_sched_barrier(0); }
#endif
    output_partial<BF16, NWP, PRE>(bufA, P.w3, wave, lane, part, &head);
    if (REC && R.noise) output_partial<BF16, NWP>(bufA, R.w3s, wave, lane, part_s);
    __syncthreads();
#ifdef ETG_PROFILE_PHASES
    { long long t = clock64(); pp[3] += t - pl; pl = t; __builtin_amdgcn_sched_barrier(0); }
#endif
    {
      const int r = tid >> 4, cidx = tid & 15;          // 256 threads = 16 rows x 16 columns
      float v = ((part[0][r][cidx] + part[1][r][cidx]) + (part[2][r][cidx] + part[3][r][cidx])) + (cidx < P.out_dim ? P.b3[cidx] : 0.0f);
      if (REC && R.noise && cidx < ETG_ACT_DIM) {
        float ls = ((part_s[0][r][cidx] + part_s[1][r][cidx]) + (part_s[2][r][cidx] + part_s[3][r][cidx])) + R.b3s[cidx];
        ls = fminf(fmaxf(ls, -20.0f), 2.0f);
        v = v + expf(ls) * R.noise[((size_t)s * K.n_env + (size_t)tile * TM + r) * ETG_ACT_DIM + cidx];
      }
      const float t = tanhf(v);
      act_lds[r][cidx] = t * act_scale;
      if (REC && cidx < ETG_ACT_DIM) R.act[((size_t)s * K.n_env + (size_t)tile * TM + r) * ETG_ACT_DIM + cidx] = t;   // the UNSCALED action (train.py:159)
    }
    __syncthreads();
    const float action = c.sub < 3 ? act_lds[4 * wave + (lane >> 4)][3 * c.leg + c.sub] : 0.0f;
#ifdef ETG_PROFILE_PHASES
    { long long t = clock64(); pp[4] += t - pl; pl = t; __builtin_amdgcn_sched_barrier(0); }
#endif
    // the step code addresses observation rows by robot index: rows of the LDS tile start at the tile's first robot.
    // Every step writes its observation to the tile (plain ds_write, no generic pointer); the last one is copied out below.
    c.row_base = tile * TM;
    const float was_alive = S.alive;
    if (!skip || c.any(was_alive > 0.5f)) {
      control_step16_core(c, K, tp, L, S, D.ring, D.etgp, action, 0.0f, obs_lds, reward, done, (float*)nullptr, (const float*)nullptr, true,
                          (float*)nullptr, (float*)nullptr, skip);
      // (a row written mid-launch gets its sensor noise at the top of the next step; only the last step's rows wait for the epilogue)
      if (skip) rollout_dead_store16(c, K, L, was_alive, done, s == n_steps - 1, false, (int)K.noise_call + s, D.base, D.leg, D.ictl);
    } else {
      reward = 0.0f; done = 1.0f;
    }
    if (c.r == 0) live_lds[4 * wave + (lane >> 4)] = skip ? was_alive : 1.0f;   // did this step write the robot's row?
#ifdef ETG_PROFILE_PHASES
    { long long t = clock64(); pp[5] += t - pl; pl = t; __builtin_amdgcn_sched_barrier(0); }
#endif
    if (REC && c.r == 0) {
      R.rew[(size_t)s * K.n_env + c.env] = reward;
      R.done[(size_t)s * K.n_env + c.env] = done > 0.5f ? 1 : 0;
    }
  }
  if (REC && c.r == 0)   // the workgroup left the loop early: the remaining steps read reward 0 / done 1 (their obs / action rows stay unwritten)
    for (int s2 = s_at; s2 < n_steps; s2++) {
      R.rew[(size_t)s2 * K.n_env + c.env] = 0.0f;
      R.done[(size_t)s2 * K.n_env + c.env] = 1;
    }
  store_ctl16(c, K, S, D.ctl, D.ictl, D.legctl);
  rollout_store16(c, K, L, S.alive, D.base, D.leg);
  __syncthreads();
  for (int idx = tid; idx < TM * ETG_OBS_DIM; idx += 256) obs[(size_t)tile * TM * ETG_OBS_DIM + idx] = obs_lds[idx];   // coalesced
#ifdef ETG_PROFILE_PHASES
  __syncthreads();
  if (tile == 0 && tid == 0) for (int k = 0; k < 8; k++) obs[k] = (float)pp[k];   // debug build: cycle breakdown over row 0
#endif
}

template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(256) k_rollout_policy16(KCfg K, DevState D, PolicyW P, int n_steps, float act_scale, float* obs) {
  using namespace pol;
  __shared__ __attribute__((aligned(16))) float bufA[TM * HS];
  __shared__ __attribute__((aligned(16))) float bufB[TM * HS];
  __shared__ float part[4][TM][16];
  __shared__ float act_lds[TM][16];
  __shared__ float obs_lds[TM * ETG_OBS_DIM];
  __shared__ float lds_par[4 * LDS16_FIELDS * 64];
  __shared__ float live_lds[TM];
  rollout_policy16_body<FLAT, true, KNEE, PLAIN, false>(K, D, P, n_steps, act_scale, obs, RecOut{}, bufA, bufB, part, nullptr, act_lds, obs_lds, lds_par, live_lds);
}

// ---- closed loop, precision 0, the 16-lane mapping: ONE WAVE per workgroup, the policy tile per wave (policy_core.h: wave_layer).
// A wave runs the actor for its own 4 robots on v_mfma_f32_4x4x1_16B_f32 and then their control step; nothing is shared with
// another wave, so there is no workgroup barrier anywhere in the loop (the __syncthreads() below are the LDS hand-overs between
// the lanes of this one wave: a wait, not a rendezvous).  REC: the recording variant (RecOut; see rollout_policy16_body).
template <bool FLAT, bool KNEE, bool PLAIN, bool REC>
__device__ __forceinline__ void rollout_policy16w_body(const KCfg& K, const DevState& D, const PolicyW& P, int n_steps, float act_scale,
                                                       float* obs, const RecOut& R, float* lds_par, float* obs4, float* abuf, float* hA,
                                                       float* hB, float* part, float (*act4)[16], float* live4, float* park) {
  using namespace pol;
  const int lane0 = threadIdx.x;
  int lane = lane0;
  const int blk = xcd_contiguous_block();             // 4 robots; the host guarantees N % 4 == 0
  GpuCtx16W<FLAT, KNEE, PLAIN> c;
  make_ctx16_fields(K, D, c, lds_par, blk, lane);
  for (int k = 0; k < PR_N; k++) lds_par[k * 64 + lane] = D.par[(size_t)k * c.NL + c.col];   // the lane's whole parameter column
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  StepCtl16<float> S = load_ctl16<float>(c, K, D.ctl, D.ictl, D.legctl);
  V3<float> fext = {0.0f, 0.0f, 0.0f};
  if (!PLAIN && K.ext_force) fext = load_fext16<float>(c, D.ctl);
  park16(park + lane0, L, S);
  float alive = S.alive;                              // (the one control variable the loop itself looks at)
  const size_t row0 = (size_t)blk * 4;
  for (int idx = lane; idx < 4 * ETG_OBS_DIM; idx += 64) obs4[idx] = obs[row0 * ETG_OBS_DIM + idx];
  if (lane < 4) live4[lane] = 1.0f;
  c.row_base = (int)row0;                             // the step code addresses observation rows by robot index
  const bool skip = K.stop_at_done != 0;
  float reward, done;
  int s_at = 0;
#ifdef ETG_PROFILE_TILE   // debugging build: cycles in the policy tile / in the control step / sweeps, per wave (written over the wave's first obs row)
  long long pt_tile = 0, pt_step = 0, pt_t = clock64();
#endif
  for (int s = 0; s < n_steps; s++, s_at = s) {
    if (skip && !c.any(alive > 0.5f)) break;          // every robot of the wave has finished: the wave is done (nobody waits for it)
    // (the lane index through an empty asm: what the tile derives from it -- LDS offsets, row addresses -- is formed here, per
    // step, instead of being kept in registers from the kernel's head through the ticks)
    lane = lane0;
    asm volatile("" : "+v"(lane));
    const int rob = lane >> 4;                        // this lane's robot in the physics mapping
    float* pk = park + lane;
    __syncthreads();
    if (K.noise_on && s > 0) {   // sensor noise on the rows the previous step wrote (the last step's: the launch's epilogue)
      if (live4[rob] > 0.5f) add_sensor_noise(K, (unsigned)(row0 + rob), K.noise_call + s - 1, lane & 15, &obs4[rob * ETG_OBS_DIM]);
      __syncthreads();
    }
    WaveRing ring;
    wave_ring_start(ring, P.w1, lane);                // the first k-groups of layer 1 arrive while the rows are staged
    // the actor's rows, zero padded to WS columns; REC: the rows it acts on
    for (int idx = lane; idx < 4 * WS; idx += 64) {
      const int r = idx / WS, col = idx - r * WS;
      abuf[idx] = col < P.in_dim ? obs4[r * ETG_OBS_DIM + P.col0 + col] : 0.0f;
    }
    if (REC)
      for (int idx = lane; idx < 4 * ETG_OBS_DIM; idx += 64) R.obs[((size_t)s * K.n_env + row0) * ETG_OBS_DIM + idx] = obs4[idx];
    __syncthreads();
    HeadW hw;
    wave_hidden12(abuf, hA, hB, ring, P.w1, P.b1, P.b2, hw, P.w3, lane);
    f32x4 mean = wave_head(hB, hw, part, lane);
    f32x4 lstd = {0.f, 0.f, 0.f, 0.f};
    if (REC && R.noise) {
      head_fetch(hw, R.w3s, lane);
      lstd = wave_head(hB, hw, part, lane);
    }
    if (lane < 12) {                                  // lane = output neuron (the actor has 12: ETG_ACT_DIM)
      const float b3 = lane < P.out_dim ? P.b3[lane] : 0.0f;
      const float b3s = (REC && R.noise && lane < ETG_ACT_DIM) ? R.b3s[lane] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float v = mean[i] + b3;
        if (REC && R.noise && lane < ETG_ACT_DIM) {
          const float ls = fminf(fmaxf(lstd[i] + b3s, -20.0f), 2.0f);
          v = v + expf(ls) * R.noise[((size_t)s * K.n_env + row0 + i) * ETG_ACT_DIM + lane];
        }
        const float t = tanhf(v);
        act4[i][lane] = t * act_scale;
        if (REC && lane < ETG_ACT_DIM) R.act[((size_t)s * K.n_env + row0 + i) * ETG_ACT_DIM + lane] = t;   // the UNSCALED action (train.py:159)
      }
    }
    __syncthreads();
    const float action = c.sub < 3 ? act4[rob][3 * c.leg + c.sub] : 0.0f;
#ifdef ETG_PROFILE_TILE
    { const long long t = clock64(); pt_tile += t - pt_t; pt_t = t; }
#endif
    // the robot state, the control variables and the tick constants come back from LDS for the step and go back after it: none
    // of them occupies a register during the tile
    c.launder_lane();
    unpark16(pk, L, S);
    S.alive = alive;
    TickPar<float> tp = load_tick_par<float>(c);
    tp.fext = fext;
    const float was_alive = alive;
    control_step16_core(c, K, tp, L, S, D.ring, D.etgp, action, 0.0f, obs4, reward, done, (float*)nullptr, (const float*)nullptr, true,
                        (float*)nullptr, (float*)nullptr, skip);
    if (skip) rollout_dead_store16(c, K, L, was_alive, done, s == n_steps - 1, false, (int)K.noise_call + s, D.base, D.leg, D.ictl);
    alive = S.alive;
    park16(pk, L, S);
#ifdef ETG_PROFILE_TILE
    { const long long t = clock64(); pt_step += t - pt_t; pt_t = t; }
#endif
    if (c.r == 0) live4[rob] = skip ? was_alive : 1.0f;   // did this step write the robot's row?
    if (REC && c.r == 0) {
      R.rew[(size_t)s * K.n_env + c.env] = reward;
      R.done[(size_t)s * K.n_env + c.env] = done > 0.5f ? 1 : 0;
    }
  }
  if (REC && c.r == 0)   // the wave left the loop early: the remaining steps read reward 0 / done 1 (their obs / action rows stay unwritten)
    for (int s2 = s_at; s2 < n_steps; s2++) {
      R.rew[(size_t)s2 * K.n_env + c.env] = 0.0f;
      R.done[(size_t)s2 * K.n_env + c.env] = 1;
    }
  c.launder_lane();
  unpark16(park + lane0, L, S);
  S.alive = alive;
  store_ctl16(c, K, S, D.ctl, D.ictl, D.legctl);
  rollout_store16(c, K, L, S.alive, D.base, D.leg);
  __syncthreads();
  for (int idx = lane0; idx < 4 * ETG_OBS_DIM; idx += 64) obs[row0 * ETG_OBS_DIM + idx] = obs4[idx];
#ifdef ETG_PROFILE_TILE
  __syncthreads();
  if (lane0 == 0) { obs[row0 * ETG_OBS_DIM + 0] = (float)pt_tile; obs[row0 * ETG_OBS_DIM + 1] = (float)pt_step; obs[row0 * ETG_OBS_DIM + 2] = (float)s_at; }
#endif
}

#define ETG_POLICY16W_LDS                                                                    \
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];                                            \
  __shared__ __attribute__((aligned(16))) float obs4[4 * ETG_OBS_DIM];                       \
  __shared__ __attribute__((aligned(16))) float abuf[4 * pol::WS];                           \
  __shared__ __attribute__((aligned(16))) float hA[4 * pol::HS];                             \
  __shared__ __attribute__((aligned(16))) float hB[4 * pol::HS];                             \
  __shared__ __attribute__((aligned(16))) float part[64 * 4];                                \
  __shared__ float park[PARK16 * BLOCK];                                                     \
  __shared__ float act4[4][16];                                                              \
  __shared__ float live4[4];
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_rollout_policy16w(KCfg K, DevState D, PolicyW P, int n_steps, float act_scale, float* obs) {
  ETG_POLICY16W_LDS
  rollout_policy16w_body<FLAT, KNEE, PLAIN, false>(K, D, P, n_steps, act_scale, obs, RecOut{}, lds_par, obs4, abuf, hA, hB, part, act4, live4, park);
}
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_rollout_policy16w_rec(KCfg K, DevState D, PolicyW P, int n_steps, float act_scale, float* obs, RecOut R) {
  ETG_POLICY16W_LDS
  rollout_policy16w_body<FLAT, KNEE, PLAIN, true>(K, D, P, n_steps, act_scale, obs, R, lds_par, obs4, abuf, hA, hB, part, act4, live4, park);
}
#undef ETG_POLICY16W_LDS

// ---- etg_step_policy (include/etgsim_step_policy.h): ONE closed-loop control step of every robot, per wave as in
// rollout_policy16w_body -- the actor on the wave's 4 observation rows (predict, or sample on the caller's noise: RecOut's
// arithmetic), then the control step of those robots with its action, as step16_body.  The step's observation goes to
// terminal_obs for every robot; AUTO: a robot whose step ended its episode restarts in the same launch (restart16) and its row
// of `obs` becomes the reset observation.  No workgroup barrier (one wave per workgroup): the __syncthreads() are the LDS
// hand-overs between the lanes of the wave.
struct StepPolOut {
  const float* noise;         // [N,12] N(0,1) draws of the stochastic actor, or NULL (predict)
  const float4* w3s;          // the packed log-std head (k_pack_head) and its bias: read when noise != NULL
  const float* b3s;
  const uint8_t* donef;       // [N] forced episode ends, or NULL
  float *act, *act_obs;       // [N,12] unscaled actions / [N,49] the rows the actor acted on: both optional
  float *term_obs, *reward;   // [N,49] the step's observation of every robot, [N]
  uint8_t* done;              // [N]
  float* info;                // [N,64], or NULL
};
// the episode records of k_collect_policy16 (all NULL in the one-step kernels): the robot's running return and 1-based episode
// step after the step and before a restart, and the bootstrap flag of the transition (replay.bootstrap_mask)
struct EpOut { float* ret; int32_t* len; float* terminal; int bootstrap_from; };
// SCAN (include/etgsim_scan_policy.h): the terrain height scan of scan_core.h computed by the wave itself.  The actor's last
// n columns are the scan of the row it acts on, and act_obs / term_obs are wide rows [N, 49 + n]: the observation, then the scan.
struct ScanPol {
  const float* points;        // [n,2]
  int n;                      // 1 .. kScanPolMax points: 4 n <= 64 lanes, one per (robot, point)
  float offset, clip;
  float* scan;                // [N,n] out: the scan columns of the rows the next step acts on
};
constexpr int kScanPolMax = 16;
// the wave's scan state in LDS (752 bytes): the points, the scan of the 4 rows the step acts on and of the 4 rows it produced
// (row stride kScanPolMax), the 4 robots' pose rows and which of them restarted
struct ScanLds { float *pts, *acted, *term; scan::Row* row; float* rst; };
// one point per lane: out[rob][j] of the robots whose pose row is in W.row; keep != NULL: only where W.rst says so, else keep's value
__device__ __forceinline__ void scan4_eval(const KCfg& K, const ScanPol& Z, const ScanLds& W, int lane, float* out, const float* keep) {
  if (lane < 4 * Z.n) {
    const int r = lane / Z.n, j = lane - r * Z.n;
    float v;
    if (keep && W.rst[r] < 0.5f) v = keep[r * kScanPolMax + j];
    else v = scan::scan_point(K, W.row[r], W.pts[2 * j], W.pts[2 * j + 1], Z.offset, Z.clip);
    out[r * kScanPolMax + j] = v;
  }
}
// launch prologue: the points, and the scan of the rows the first step acts on, from the live state in D.base (what
// etg_height_scan reads: state_pose / make_row / scan_point) -- no input buffer that could be stale
__device__ __forceinline__ void scan4_begin(const KCfg& K, const DevState& D, const ScanPol& Z, const ScanLds& W, int lane, int row0) {
  if (lane < 2 * Z.n) W.pts[lane] = Z.points[lane];
  if (lane < 4) {
    float p[4];
    scan::state_pose(D.base, K.n_env, row0 + lane, p);
    W.row[lane] = scan::make_row(p, row0 + lane);
  }
  __syncthreads();
  scan4_eval(K, Z, W, lane, W.acted, nullptr);
  __syncthreads();
}
// launch epilogue: the scan columns of the rows the next step acts on
__device__ __forceinline__ void scan4_end(const ScanPol& Z, const ScanLds& W, int lane, int row0) {
  if (lane < 4 * Z.n) {
    const int r = lane / Z.n, j = lane - r * Z.n;
    Z.scan[(size_t)row0 * Z.n + lane] = W.acted[r * kScanPolMax + j];
  }
}
// LOOP (k_collect_policy16 calls the body once per control step): the lane and block indices go through an empty asm, so what the
// body derives from them is formed anew in every iteration instead of being hoisted and kept in registers through the ticks
template <bool FLAT, bool KNEE, bool PLAIN, bool AUTO, bool LOOP = false, bool SCAN = false>
__device__ __forceinline__ void step_policy16_body(const KCfg& K, const DevState& D, const PolicyW& P, float act_scale, float* obs,
                                                   const StepPolOut& O, const NextDyn& NX, float* lds_par, float* obs4, float* abuf,
                                                   float* hA, float* hB, float* part, float (*act4)[16],
                                                   const EpOut E = EpOut{nullptr, nullptr, nullptr, 0},
                                                   const ScanPol Z = ScanPol{nullptr, 0, 0.0f, 0.0f, nullptr},
                                                   const ScanLds W = ScanLds{nullptr, nullptr, nullptr, nullptr, nullptr}) {
  using namespace pol;
  int lane = threadIdx.x;
  int blk = xcd_contiguous_block();                   // 4 robots; the host guarantees N % 16 == 0 (the grid is N / 4 exactly)
  if (LOOP) asm volatile("" : "+v"(lane), "+s"(blk));
  const size_t row0 = (size_t)blk * 4;
  // the actor: its rows, zero padded to WS columns, and (optionally) a copy of the rows for the replay memory
  WaveRing ring;
  wave_ring_start(ring, P.w1, lane);                  // the first k-groups of layer 1 arrive while the rows are staged
  for (int idx = lane; idx < 4 * ETG_OBS_DIM; idx += 64) obs4[idx] = obs[row0 * ETG_OBS_DIM + idx];
  __syncthreads();
  if constexpr (SCAN) {                               // (W.acted: the launch prologue's, or the previous iteration's)
    const int nobs = P.in_dim - Z.n, wide = ETG_OBS_DIM + Z.n;
    for (int idx = lane; idx < 4 * WS; idx += 64) {
      const int r = idx / WS, col = idx - r * WS;
      abuf[idx] = col < nobs ? obs4[r * ETG_OBS_DIM + P.col0 + col] : col < P.in_dim ? W.acted[r * kScanPolMax + col - nobs] : 0.0f;
    }
    for (int idx = lane; idx < 4 * wide; idx += 64) {
      const int r = idx / wide, col = idx - r * wide;
      O.act_obs[row0 * wide + idx] = col < ETG_OBS_DIM ? obs4[r * ETG_OBS_DIM + col] : W.acted[r * kScanPolMax + col - ETG_OBS_DIM];
    }
  } else {
    for (int idx = lane; idx < 4 * WS; idx += 64) {
      const int r = idx / WS, col = idx - r * WS;
      abuf[idx] = col < P.in_dim ? obs4[r * ETG_OBS_DIM + P.col0 + col] : 0.0f;
    }
    if (O.act_obs)
      for (int idx = lane; idx < 4 * ETG_OBS_DIM; idx += 64) O.act_obs[row0 * ETG_OBS_DIM + idx] = obs4[idx];
  }
  __syncthreads();
  HeadW hw;
  wave_hidden12(abuf, hA, hB, ring, P.w1, P.b1, P.b2, hw, P.w3, lane);
  f32x4 mean = wave_head(hB, hw, part, lane);
  f32x4 lstd = {0.f, 0.f, 0.f, 0.f};
  if (O.noise) {
    head_fetch(hw, O.w3s, lane);
    lstd = wave_head(hB, hw, part, lane);
  }
  if (lane < ETG_ACT_DIM) {                           // lane = output neuron
    const float b3 = P.b3[lane];
    const float b3s = O.noise ? O.b3s[lane] : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      float v = mean[i] + b3;
      if (O.noise) {
        const float ls = fminf(fmaxf(lstd[i] + b3s, -20.0f), 2.0f);
        v = v + expf(ls) * O.noise[(row0 + i) * ETG_ACT_DIM + lane];
      }
      const float t = tanhf(v);
      act4[i][lane] = t * act_scale;
      if (O.act) O.act[(row0 + i) * ETG_ACT_DIM + lane] = t;   // the UNSCALED action (train.py:159)
    }
  }
  __syncthreads();
  // the control step (step16_body with the action from LDS and the observation rows in LDS: c.row_base)
  GpuCtx16T<FLAT, KNEE, PLAIN> c;
  make_ctx16_fields(K, D, c, lds_par, blk, lane);
  float stg[kNStaged16];
  stage16_issue(D, c, stg);
  State16<float> L = load_state16<float>(c, D.base, D.leg);
  StepCtl16<float> S = load_ctl16<float>(c, K, D.ctl, D.ictl, D.legctl);
  TickPar<float> tp = load_tick_par<float>(c);
  if (!PLAIN && K.ext_force) tp.fext = load_fext16<float>(c, D.ctl);
  const float act = c.sub < 3 ? act4[lane >> 4][3 * c.leg + c.sub] : 0.0f;
  const float dflag = O.donef ? (float)O.donef[c.env] : 0.0f;
  stage16_commit(c, stg);
  c.row_base = (int)row0;                             // observation rows: obs4; info rows: through a pointer moved by the same rows
  float r, d;
  control_step16_core(c, K, tp, L, S, D.ring, D.etgp, act, dflag, obs4, r, d, O.info ? O.info + row0 * ETG_INFO_DIM : (float*)nullptr);
  store_ctl16(c, K, S, D.ctl, D.ictl, D.legctl);
  if (E.ret && c.r == 0) {
    const int len = (int)S.len;
    E.ret[c.env] = S.ret;
    E.len[c.env] = len;
    E.terminal[c.env] = (len >= E.bootstrap_from || d <= 0.5f) ? 1.0f : 0.0f;
  }
  // SCAN: the scan of the pose the step produced, from the state itself (what store_state16 is about to write to D.base)
  if constexpr (SCAN)
    if (c.r == 0) W.row[lane >> 4] = scan::row_of_base(L.p.x, L.p.y, L.p.z, L.qx, L.qy, L.qz, L.qw, c.env);
  __syncthreads();
  if constexpr (SCAN) {
    scan4_eval(K, Z, W, lane, W.term, nullptr);
    __syncthreads();
    const int wide = ETG_OBS_DIM + Z.n;
    for (int idx = lane; idx < 4 * wide; idx += 64) {
      const int r = idx / wide, col = idx - r * wide;
      O.term_obs[row0 * wide + idx] = col < ETG_OBS_DIM ? obs4[r * ETG_OBS_DIM + col] : W.term[r * kScanPolMax + col - ETG_OBS_DIM];
    }
  } else {
    for (int idx = lane; idx < 4 * ETG_OBS_DIM; idx += 64) O.term_obs[row0 * ETG_OBS_DIM + idx] = obs4[idx];
  }
  if (AUTO) {
    __syncthreads();                                  // the rows are read before a restart writes its reset row over them
    if (d > 0.5f) restart16(c, K, D, NX, L, obs4);    // whole 16-lane rows take this branch together (d is the robot's)
  }
  if constexpr (SCAN) {   // the next step's acted scan: the step's own, or -- a restarted robot -- the scan of its reset state
    const bool rst = AUTO && d > 0.5f;
    if (c.r == 0) {
      W.rst[lane >> 4] = rst ? 1.0f : 0.0f;
      if (rst) W.row[lane >> 4] = scan::row_of_base(L.p.x, L.p.y, L.p.z, L.qx, L.qy, L.qz, L.qw, c.env);
    }
    __syncthreads();
    scan4_eval(K, Z, W, lane, W.acted, W.term);
  }
  store_state16(c, D.base, D.leg, L);
  if (c.r == 0) {
    O.reward[c.env] = r;
    O.done[c.env] = d > 0.5f ? 1 : 0;
  }
  __syncthreads();
  for (int idx = lane; idx < 4 * ETG_OBS_DIM; idx += 64) obs[row0 * ETG_OBS_DIM + idx] = obs4[idx];
}
#define ETG_SCAN_POLICY16_LDS                                                                \
  __shared__ float scan_pts[2 * kScanPolMax];                                                \
  __shared__ float scan_acted[4 * kScanPolMax];                                              \
  __shared__ float scan_term[4 * kScanPolMax];                                               \
  __shared__ scan::Row scan_row[4];                                                          \
  __shared__ float scan_rst[4];                                                              \
  const ScanLds W = {scan_pts, scan_acted, scan_term, scan_row, scan_rst};
#define ETG_STEP_POLICY16_LDS                                                                \
  __shared__ float lds_par[LDS16_FIELDS * BLOCK];                                            \
  __shared__ __attribute__((aligned(16))) float obs4[4 * ETG_OBS_DIM];                       \
  __shared__ __attribute__((aligned(16))) float abuf[4 * pol::WS];                           \
  __shared__ __attribute__((aligned(16))) float hA[4 * pol::HS];                             \
  __shared__ __attribute__((aligned(16))) float hB[4 * pol::HS];                             \
  __shared__ __attribute__((aligned(16))) float part[64 * 4];                                \
  __shared__ float act4[4][16];
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_step_policy16(KCfg K, DevState D, PolicyW P, float act_scale, float* obs, StepPolOut O) {
  ETG_STEP_POLICY16_LDS
  step_policy16_body<FLAT, KNEE, PLAIN, false>(K, D, P, act_scale, obs, O, NextDyn{nullptr, nullptr, nullptr}, lds_par, obs4, abuf, hA, hB, part, act4);
}
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_step_policy16_ar(KCfg K, DevState D, PolicyW P, float act_scale, float* obs, StepPolOut O, NextDyn NX) {
  ETG_STEP_POLICY16_LDS
  step_policy16_body<FLAT, KNEE, PLAIN, true>(K, D, P, act_scale, obs, O, NX, lds_par, obs4, abuf, hA, hB, part, act4);
}
// ... with the scan columns (include/etgsim_scan_policy.h): the same body with SCAN, between the prologue that scans the live
// state and the epilogue that hands the next step's scan columns out
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_step_policy16_scan(KCfg K, DevState D, PolicyW P, float act_scale, float* obs, StepPolOut O, ScanPol Z) {
  ETG_STEP_POLICY16_LDS
  ETG_SCAN_POLICY16_LDS
  const int row0 = xcd_contiguous_block() * 4;
  scan4_begin(K, D, Z, W, threadIdx.x, row0);
  step_policy16_body<FLAT, KNEE, PLAIN, false, false, true>(K, D, P, act_scale, obs, O, NextDyn{nullptr, nullptr, nullptr}, lds_par, obs4, abuf, hA,
                                                            hB, part, act4, EpOut{nullptr, nullptr, nullptr, 0}, Z, W);
  scan4_end(Z, W, threadIdx.x, row0);                 // (the body ends behind a __syncthreads() that follows its last write of W.acted)
}
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_step_policy16_scan_ar(KCfg K, DevState D, PolicyW P, float act_scale, float* obs, StepPolOut O, NextDyn NX,
                                                                 ScanPol Z) {
  ETG_STEP_POLICY16_LDS
  ETG_SCAN_POLICY16_LDS
  const int row0 = xcd_contiguous_block() * 4;
  scan4_begin(K, D, Z, W, threadIdx.x, row0);
  step_policy16_body<FLAT, KNEE, PLAIN, true, false, true>(K, D, P, act_scale, obs, O, NX, lds_par, obs4, abuf, hA, hB, part, act4,
                                                           EpOut{nullptr, nullptr, nullptr, 0}, Z, W);
  scan4_end(Z, W, threadIdx.x, row0);
}

// ---- etg_collect_policy (include/etgsim_collect.h): n_steps closed-loop control steps WITH restarts in one launch.  A wave
// stays with its 4 robots for the whole launch and never waits for another wave, so a robot that kneels for a few steps costs
// its own wave's time only.  Every iteration is step_policy16_body<AUTO> on the step's slices of the [n_steps][N][...] records,
// and the state is carried from one iteration to the next exactly as a launch boundary carries it: the body ends with
// store_ctl16 / restart16 / store_state16 and the rows of obs4 in `obs`, and begins with load_state16 / load_ctl16 and the rows
// of `obs` (L2-resident round trips of the wave's own lines, next to 13 physics ticks).  So one launch of K steps leaves bit for
// bit what K launches of one step leave.  A restart finds no prepared next-episode dynamics (the host refuses such a handle:
// a second restart inside the launch would find none), hence the null NextDyn.
struct CollectOut {
  const float* noise;         // [K,N,12] N(0,1) draws, or NULL (predict)
  const float4* w3s;          // the packed log-std head and its bias: read when noise != NULL
  const float* b3s;
  const uint8_t* donef;       // [K,N] forced episode ends, or NULL
  float *obs, *act, *rew;     // [K,N,49] the rows acted on, [K,N,12] unscaled actions, [K,N]
  uint8_t* done;              // [K,N]
  float *next_obs, *terminal, *ep_ret;   // [K,N,49] the step's rows before any restart, [K,N], [K,N]
  int32_t* ep_len;            // [K,N]
  float* info;                // [K,N,64], or NULL (etg_collect_policy passes NULL).  A run-time value on purpose: with a constant NULL
                              // the reward terms lose their second use, the compiler contracts them into the reward's sum, and the
                              // rewards stop being bit-equal to k_step_policy16_ar's (collect_continuous: chunked == per step)
};
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_collect_policy16(KCfg K, DevState D, PolicyW P, float act_scale, float* obs, CollectOut R,
                                                             int n_steps, int bootstrap_from) {
  ETG_STEP_POLICY16_LDS
  const size_t N = K.n_env;
  for (int s = 0; s < n_steps; s++) {
    const size_t at = (size_t)s * N;
    const StepPolOut O = {R.noise ? R.noise + at * ETG_ACT_DIM : nullptr, R.w3s, R.b3s, R.donef ? R.donef + at : nullptr,
                          R.act + at * ETG_ACT_DIM, R.obs + at * ETG_OBS_DIM, R.next_obs + at * ETG_OBS_DIM, R.rew + at, R.done + at,
                          R.info ? R.info + at * ETG_INFO_DIM : nullptr};
    step_policy16_body<FLAT, KNEE, PLAIN, true, true>(K, D, P, act_scale, obs, O, NextDyn{nullptr, nullptr, nullptr}, lds_par, obs4, abuf, hA, hB,
                                                      part, act4, EpOut{R.ep_ret + at, R.ep_len + at, R.terminal + at, bootstrap_from});
    __syncthreads();                                  // the rows of obs4 are out before the next iteration stages them again
  }
}
// ... with the scan columns: rec obs / next_obs are wide rows [K,N,49+n], and the 4 x n values of W.acted are carried from one
// iteration to the next in LDS, as the rows of obs4 are carried in `obs`
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(BLOCK) k_collect_policy16_scan(KCfg K, DevState D, PolicyW P, float act_scale, float* obs, CollectOut R,
                                                                  int n_steps, int bootstrap_from, ScanPol Z) {
  ETG_STEP_POLICY16_LDS
  ETG_SCAN_POLICY16_LDS
  const size_t N = K.n_env, wide = ETG_OBS_DIM + Z.n;
  const int row0 = xcd_contiguous_block() * 4;
  scan4_begin(K, D, Z, W, threadIdx.x, row0);
  for (int s = 0; s < n_steps; s++) {
    const size_t at = (size_t)s * N;
    const StepPolOut O = {R.noise ? R.noise + at * ETG_ACT_DIM : nullptr, R.w3s, R.b3s, R.donef ? R.donef + at : nullptr,
                          R.act + at * ETG_ACT_DIM, R.obs + at * wide, R.next_obs + at * wide, R.rew + at, R.done + at,
                          R.info ? R.info + at * ETG_INFO_DIM : nullptr};
    step_policy16_body<FLAT, KNEE, PLAIN, true, true, true>(K, D, P, act_scale, obs, O, NextDyn{nullptr, nullptr, nullptr}, lds_par, obs4, abuf, hA,
                                                            hB, part, act4, EpOut{R.ep_ret + at, R.ep_len + at, R.terminal + at, bootstrap_from},
                                                            Z, W);
    __syncthreads();
  }
  scan4_end(Z, W, threadIdx.x, row0);
}
#undef ETG_SCAN_POLICY16_LDS
#undef ETG_STEP_POLICY16_LDS

// Closed loop on the 4-lanes-per-robot mapping (the mapping of every batch above 4096 robots): a workgroup of 4 waves owns
// 64 robots (16 per wave, one leg per lane).  The policy runs over TWO stacked 16-row tiles at a time (hidden_layer_rt): every
// weight fragment fetched from L2 feeds two MFMAs, so the weight delivery per robot is half that of k_rollout_policy16, and a
// workgroup does two such passes per control step.  Activations of the 32 rows of a pass, the 64 observation rows and the
// actions stay in LDS; each wave then runs the control step of its 16 robots.  Same arithmetic per row as the 16-lane kernel.
template <bool FLAT, bool BF16, bool PLAIN, int BODY = 0>
__global__ void __launch_bounds__(256) k_rollout_policy4(KCfg K, DevState D, PolicyW P, int n_steps, float act_scale, float* obs) {
  using namespace pol;
  constexpr int NWP = 4, RT = 2, ROWS = 64;
  __shared__ __attribute__((aligned(16))) float bufA[RT * TM * HS];
  __shared__ __attribute__((aligned(16))) float bufB[RT * TM * HS];
  __shared__ float part[NWP][RT * TM][16];
  __shared__ float act_lds[ROWS][16];
  __shared__ float obs_lds[ROWS * ETG_OBS_DIM];
  __shared__ float lds_par[NWP][PR_N * 64];
  __shared__ float live_lds[ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = xcd_contiguous_block();            // 64 robots; the host guarantees N % 64 == 0
  GpuCtxT<FLAT, PLAIN, BODY> c;
  c.gid = tile * 256 + tid;
  c.N = K.n_env;
  c.NL = 4 * K.n_env;
  c.env = c.gid >> 2;
  c.lane = c.gid & 3;
  stage_params_wave(c, D, lds_par[wave], lane);
  LaneState<float> L = load_state<float>(c, D.base, D.leg);
  StepCtl4<float> S = load_ctl4<float>(c, K, D.ctl, D.ictl, D.legctl);
  TickPar4<float> tp = load_tick_par4<float>(c);
  V3<float> fext = {0.0f, 0.0f, 0.0f};
  if (!PLAIN && K.ext_force) fext = {c.ld_env(D.ctl, CT_FEXT + 0) + c.ld_env(D.ctl, CT_PUSH + 0), c.ld_env(D.ctl, CT_FEXT + 1) + c.ld_env(D.ctl, CT_PUSH + 1),
                                     c.ld_env(D.ctl, CT_FEXT + 2) + c.ld_env(D.ctl, CT_PUSH + 2)};
  for (int idx = tid; idx < ROWS * ETG_OBS_DIM; idx += 256) obs_lds[idx] = obs[(size_t)tile * ROWS * ETG_OBS_DIM + idx];
  c.row_base = tile * ROWS;
  float reward, done;
  const bool skip = K.stop_at_done != 0;     // (see rollout_policy16_body)
  if (tid < ROWS) live_lds[tid] = 1.0f;
  for (int s = 0; s < n_steps; s++) {
    if (skip) {
      if (!__syncthreads_or(S.alive > 0.5f)) break;
    } else {
      __syncthreads();
    }
    if (K.noise_on && s > 0) {   // sensor noise on the rows the previous step wrote to LDS (the last ones: the launch's epilogue)
      for (int idx = tid; idx < ROWS * 16; idx += 256)
        if (live_lds[idx >> 4] > 0.5f)
          add_sensor_noise(K, tile * ROWS + (idx >> 4), K.noise_call + s - 1, idx & 15, &obs_lds[(idx >> 4) * ETG_OBS_DIM]);
      __syncthreads();
    }
    for (int pass = 0; pass < ROWS / (RT * TM); pass++) {
      const int r0 = pass * RT * TM;
      for (int idx = tid; idx < RT * TM * 64; idx += 256) {   // observation rows of the pass, zero padded to the 64-wide K of layer 1
        const int r = idx >> 6, col = idx & 63;
        bufA[r * HS + col] = col < P.in_dim ? obs_lds[(r0 + r) * ETG_OBS_DIM + P.col0 + col] : 0.0f;
      }
      __syncthreads();
      hidden_layer_rt<BF16, 4, NWP, RT>(bufA, P.w1, P.b1, bufB, wave, lane);
      __syncthreads();
      hidden_layer_rt<BF16, HID / 16, NWP, RT>(bufB, P.w2, P.b2, bufA, wave, lane);
      __syncthreads();
      output_partial_rt<BF16, NWP, RT>(bufA, P.w3, wave, lane, part);
      __syncthreads();
      for (int idx = tid; idx < RT * TM * 16; idx += 256) {
        const int r = idx >> 4, cidx = idx & 15;
        const float v = ((part[0][r][cidx] + part[1][r][cidx]) + (part[2][r][cidx] + part[3][r][cidx])) + (cidx < P.out_dim ? P.b3[cidx] : 0.0f);
        act_lds[r0 + r][cidx] = tanhf(v) * act_scale;
      }
      __syncthreads();
    }
    const int rl = 16 * wave + (lane >> 2), leg = lane & 3;
    const float act[3] = {act_lds[rl][3 * leg + 0], act_lds[rl][3 * leg + 1], act_lds[rl][3 * leg + 2]};
    const float was_alive = S.alive;
    if (!skip || c.any(was_alive > 0.5f)) {
      control_step_core(c, K, tp, fext, L, S, D.ring, D.etgp, act, 0.0f, obs_lds, reward, done, (float*)nullptr, (const float*)nullptr, true,
                        (float*)nullptr, (float*)nullptr, skip);
      if (skip) rollout_dead_store(c, K, L, was_alive, done, s == n_steps - 1, false, (int)K.noise_call + s, D.base, D.leg, D.ictl);
    }
    if (c.lane == 0) live_lds[rl] = skip ? was_alive : 1.0f;
  }
  store_ctl4(c, K, S, D.ctl, D.ictl, D.legctl);
  rollout_store(c, K, L, S.alive, D.base, D.leg);
  __syncthreads();
  for (int idx = tid; idx < ROWS * ETG_OBS_DIM; idx += 256) obs[(size_t)tile * ROWS * ETG_OBS_DIM + idx] = obs_lds[idx];   // coalesced
}

// the recording variant of k_rollout_policy16 (etg_rollout_policy_record): the same body with REC = true
template <bool FLAT, bool KNEE, bool PLAIN>
__global__ void __launch_bounds__(256) k_rollout_policy16_rec(KCfg K, DevState D, PolicyW P, int n_steps, float act_scale, float* obs, RecOut R) {
  using namespace pol;
  __shared__ __attribute__((aligned(16))) float bufA[TM * HS];
  __shared__ __attribute__((aligned(16))) float bufB[TM * HS];
  __shared__ float part[4][TM][16];
  __shared__ float part_s[4][TM][16];   // log-std head (stochastic actor only)
  __shared__ float act_lds[TM][16];
  __shared__ float obs_lds[TM * ETG_OBS_DIM];
  __shared__ float lds_par[4 * LDS16_FIELDS * 64];
  __shared__ float live_lds[TM];
  rollout_policy16_body<FLAT, true, KNEE, PLAIN, true>(K, D, P, n_steps, act_scale, obs, R, bufA, bufB, part, part_s, act_lds, obs_lds, lds_par, live_lds);
}

// Gaussian sensor noise on freshly written observation rows: one thread per (robot, channel).  A separate tiny
// kernel so that the step kernels' code (and register allocation) is the same with and without noise.
#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void k_add_noise(KCfg K, unsigned call, const uint8_t* mask, int invert, float* obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = i >> 4;
  if (env >= K.n_env || (mask && (mask[env] != 0) == (invert != 0))) return;   // mask: rows to touch (or, inverted, to leave)
  add_sensor_noise(K, env, call, i & 15, obs + (size_t)env * ETG_OBS_DIM);
}

__global__ void k_add_noise_range(KCfg K, unsigned call, int env0, int count, float* obs) {   // etg_step_range's rows
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if ((i >> 4) >= count) return;
  const int env = env0 + (i >> 4);
  add_sensor_noise(K, env, call, i & 15, obs + (size_t)env * ETG_OBS_DIM);
}

// the epilogue of a fused rollout launch under KCfg.stop_at_done: rows were written at different steps (a robot's last one when
// its episode ended), each noted its stream position in ictl[IC_OBS_CALL]; rows noted in [first, first + n) get their noise
__global__ void k_add_noise_rows(KCfg K, DevState D, unsigned first, unsigned n, float* obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = i >> 4;
  if (env >= K.n_env) return;
  const unsigned call = (unsigned)D.ictl[(size_t)IC_OBS_CALL * K.n_env + env];
  if (call - first >= n) return;
  add_sensor_noise(K, env, call, i & 15, obs + (size_t)env * ETG_OBS_DIM);
}

// external force rows [N,3] -> the three SoA columns ctl[CT_FEXT + k][N]
__global__ void k_set_fext(KCfg K, DevState D, const float* force) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K.n_env) return;
  for (int k = 0; k < 3; k++) D.ctl[(size_t)(CT_FEXT + k) * K.n_env + i] = force[(size_t)i * 3 + k];
}
#endif

// counter-based uniform in [0,1): a 64-bit mix (splitmix64 finaliser) of (seed, robot, call, stream)
__device__ __forceinline__ float push_uniform(unsigned long long seed, unsigned env, unsigned long long call, unsigned k) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (((unsigned long long)env << 32 | k) + 0xD1B54A32D192ED03ull * (call + 1));
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}
#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void k_random_pushes(KCfg K, DevState D, unsigned long long seed, unsigned long long call, float prob, int duration,
                                float fmin, float fmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = K.n_env;
  if (i >= N) return;
  int left = D.ictl[(size_t)IC_PUSH_LEFT * N + i];
  float fx = D.ctl[(size_t)(CT_PUSH + 0) * N + i], fy = D.ctl[(size_t)(CT_PUSH + 1) * N + i];
  if (left > 0) {
    left--;
    if (left == 0) { fx = 0.0f; fy = 0.0f; }
  } else if (push_uniform(seed, i, call, 0) < prob) {
    const float ang = 6.283185307179586f * push_uniform(seed, i, call, 1);
    const float mag = fmin + (fmax - fmin) * push_uniform(seed, i, call, 2);
    fx = mag * cosf(ang); fy = mag * sinf(ang);
    left = duration;
  }
  D.ictl[(size_t)IC_PUSH_LEFT * N + i] = left;
  D.ctl[(size_t)(CT_PUSH + 0) * N + i] = fx;
  D.ctl[(size_t)(CT_PUSH + 1) * N + i] = fy;
  D.ctl[(size_t)(CT_PUSH + 2) * N + i] = 0.0f;
}
__global__ void k_clear_pushes(KCfg K, DevState D, const uint8_t* mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = K.n_env;
  if (i >= N || (mask && !mask[i])) return;
  D.ictl[(size_t)IC_PUSH_LEFT * N + i] = 0;
  for (int k = 0; k < 3; k++) D.ctl[(size_t)(CT_PUSH + k) * N + i] = 0.0f;   // the set force (CT_FEXT) stays
}

// copy out the per-robot episode accumulators (return, length) kept in ctl[]
__global__ void k_episode_stats(KCfg K, DevState D, float* ret, int* len) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K.n_env) return;
  if (ret) ret[i] = D.ctl[(size_t)CT_RET * K.n_env + i];
  if (len) len[i] = (int)D.ctl[(size_t)CT_LEN * K.n_env + i];
}

__global__ void __launch_bounds__(BLOCK) k_get_state(KCfg K, DevState D, float* st) {
  GpuCtxT<true> c;
  if (!make_ctx(K, c)) return;
  LaneState<float> L = load_state<float>(c, D.base, D.leg);
  get_state_quad(c, L, st);
}
__global__ void __launch_bounds__(BLOCK) k_set_state(KCfg K, DevState D, const float* st) {
  GpuCtxT<true> c;
  if (!make_ctx(K, c)) return;
  LaneState<float> L;
  set_state_quad(c, st, L, D.ring, D.ctl, D.ictl, K.settle_ticks + RING);
  store_state(c, D.base, D.leg, L);
}

// leg FK + analytic Jacobian through the tick's own leg_geometry (etg_leg_kinematics): 4 joint-angle rows per
// wave, lane r = 4*leg + sub of a 16-lane row like the step kernels.  Sub-lane s < 3 writes component s of the
// foot position (base frame) and row s of d foot / d (hip, thigh, calf): the columns are the k1, k2, k3 lever
// arms the contact rows of physics_tick16 are built from, evaluated at the foot centre.
__global__ void __launch_bounds__(BLOCK) k_leg_kin(KCfg K, ModelF M, const float* q, int n, float* foot, float* jac) {
  GpuCtx16T<true> c;
  const int lane = threadIdx.x;
  const int row = blockIdx.x * 4 + (lane >> 4);
  const bool live = row < n;
  const int rr = live ? row : n - 1;          // keep every quad complete for the DPP exchanges
  c.r = lane & 15; c.leg = c.r >> 2; c.sub = c.r & 3; c.sc = c.sub < 2 ? c.sub : 2;
  const float qo = c.sub < 3 ? q[(size_t)rr * 12 + 3 * c.leg + c.sub] : 0.0f;
  const V3<float> o1 = {M.hip_origin[c.leg][0], M.hip_origin[c.leg][1], M.hip_origin[c.leg][2]};
  const LegGeo<float> g = leg_geometry(c, K, o1, M.thigh_y[c.leg], qo);
  const V3<float> xax = {1.0f, 0.0f, 0.0f};
  const V3<float> k1 = cross(xax, g.pf - g.o1), k2 = cross(g.yax, g.pf - g.o2), k3 = cross(g.yax, g.pf - g.o3);
  if (!live || c.sub == 3) return;
  const int s = c.sub;
  foot[(size_t)row * 12 + 3 * c.leg + s] = s == 0 ? g.pf.x : s == 1 ? g.pf.y : g.pf.z;
  if (jac) {
    float* J = jac + (((size_t)row * 4 + c.leg) * 3 + s) * 3;
    J[0] = s == 0 ? k1.x : s == 1 ? k1.y : k1.z;
    J[1] = s == 0 ? k2.x : s == 1 ? k2.y : k2.z;
    J[2] = s == 0 ? k3.x : s == 1 ? k3.y : k3.z;
  }
}

// optional sensors (include/etgsim.h ETG_EXTRA_*): column `col` of a robot's row, from its observation row `orow` [49] and the
// state the column reads through `src` -- step(): the episode step index of the row (IC_STEP), dyn(k): its dynamic_param row,
// force(k): the trunk force (set + random push).  The live state (ExtraLive: etg_extra_sensors) or what a restart overwrote
// (ExtraCtx: a terminal_ctx row, etg_extra_sensors_terminal).
struct ExtraLive {
  const DevState& D;
  int env, N;
  __device__ int step() const { return D.ictl[(size_t)IC_STEP * N + env]; }
  __device__ float dyn(int k) const { return D.dyn[(size_t)env * ETG_DYN_DIM + k]; }
  __device__ float force(int k) const { return D.ctl[(size_t)(CT_FEXT + k) * N + env] + D.ctl[(size_t)(CT_PUSH + k) * N + env]; }
};
struct ExtraCtx {
  const float* row;   // [ETG_TERM_CTX_DIM]
  __device__ int step() const { return (int)row[ETG_TERM_STEP]; }
  __device__ float dyn(int k) const { return row[ETG_TERM_DYN + k]; }
  __device__ float force(int k) const { return row[ETG_TERM_FORCE + k]; }
};
template <class Src>
__device__ __forceinline__ float extra_sensor(const KCfg& K, const ModelF& M, int col, const float* orow, const Src& src) {
  float v = 0.0f;
  if (col < ETG_EXTRA_FOOTPOSE) {            // RBF activations at the ETG time of the row's observation
    const int k = src.step();
    const float t = (float)k * K.etg_dt;
    const float x0 = K.etg_amp * sinf(K.etg_phase0 + t * K.etg_omega), x1 = K.etg_amp * sinf(K.etg_phase1 + t * K.etg_omega);
    const float d0 = x0 - K.etg_u[col][0], d1 = x1 - K.etg_u[col][1];
    v = expf(-(d0 * d0 + d1 * d1) / K.etg_sigma_sq);
  } else if (col < ETG_EXTRA_DYNAMIC) {      // foot_positions_in_base_frame (a1.py:113-140) of the OBSERVED motor angles
    const int j = col - ETG_EXTRA_FOOTPOSE, leg = j / 3, k = j % 3;
    float a[3];
    for (int m = 0; m < 3; m++) {
      const float o = orow[13 + 3 * leg + m];
      a[m] = K.obs_normal ? o * 0.1f + M.pose[3 * leg + m] : o;
    }
    const float l_hip = M.thigh_y[leg], lu = K.upper_len, ll = K.lower_len;
    const float dist = sqrtf(lu * lu + ll * ll + 2.0f * lu * ll * cosf(a[2]));
    const float sw = a[1] + 0.5f * a[2];
    const float ox = -dist * sinf(sw), oz = -dist * cosf(sw), oy = l_hip;
    const float p[3] = {ox, cosf(a[0]) * oy - sinf(a[0]) * oz, sinf(a[0]) * oy + cosf(a[0]) * oz};
    v = p[k] + M.hip_origin[leg][k];
  } else if (col < ETG_EXTRA_FORCE) {        // inverse of param2dynamic_dict's affine maps (train.py:112-126)
    const int k = col - ETG_EXTRA_DYNAMIC;
    const float d = src.dyn(k);
    if (k == 0) v = (d - 40.0f) * 0.1f;
    else if (k == 1) v = (d - 0.2f) * 0.1f;
    else if (k == 2) v = d - 1.5f;
    else if (k < 21) v = d - 1.0f;
    else if (k < 33) v = (d - 80.0f) * 0.025f;
    else if (k < 45) { const float kd0 = ((k - 33) % 3 == 0) ? 1.0f : 2.0f; v = (d - kd0) / kd0; }
    else { const float g0[3] = {0.0f, 0.0f, -10.0f}, gs[3] = {2.0f, 2.0f, 10.0f}; v = (d - g0[k - 45]) / gs[k - 45]; }
  } else if (col < ETG_EXTRA_FORCE + 3) {
    v = src.force(col - ETG_EXTRA_FORCE);
  }
  return v;
}

// one thread per (robot, column)
__global__ void k_extra_sensors(KCfg K, ModelF M, DevState D, const float* obs, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = i / ETG_EXTRA_DIM, col = i % ETG_EXTRA_DIM;
  const int N = K.n_env;
  if (env >= N) return;
  out[(size_t)env * ETG_EXTRA_DIM + col] = extra_sensor(K, M, col, obs + (size_t)env * ETG_OBS_DIM, ExtraLive{D, env, N});
}

// the columns of the terminal rows (etg_extra_sensors_terminal): a robot that went on reads the live state, a restarted one
// (done) its terminal_ctx row
__global__ void k_extra_sensors_terminal(KCfg K, ModelF M, DevState D, const float* obs, const float* ctx, const uint8_t* done, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = i / ETG_EXTRA_DIM, col = i % ETG_EXTRA_DIM;
  const int N = K.n_env;
  if (env >= N) return;
  const float* orow = obs + (size_t)env * ETG_OBS_DIM;
  out[(size_t)env * ETG_EXTRA_DIM + col] = done[env] ? extra_sensor(K, M, col, orow, ExtraCtx{ctx + (size_t)env * ETG_TERM_CTX_DIM})
                                                     : extra_sensor(K, M, col, orow, ExtraLive{D, env, N});
}

// the rows of `obs` of the robots that went on in a 4-lane k_step_ar launch with T.obs (step4_body): their terminal rows
__global__ void __launch_bounds__(256) k_term_rows(KCfg K, const float* tobs, const uint8_t* done, float* obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K.n_env * ETG_OBS_DIM || done[i / ETG_OBS_DIM]) return;
  obs[i] = tobs[i];
}

// the terminal_ctx rows of the robots a masked etg_reset is about to restart (etg_step_autoreset_terminal without a cached
// settle for every robot): the live state after the step, before the reset
__global__ void __launch_bounds__(256) k_term_ctx(KCfg K, DevState D, const uint8_t* done, float* ctx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = i >> 4;
  if (env >= K.n_env || !done[env]) return;
  term_ctx_store(K, D, env, i & 15, 16, D.ictl[(size_t)IC_STEP * K.n_env + env], ctx);
}
#endif

// ---- the tick kernels' instantiations, one row per kernel family, one SLOT per instantiation.  A slot belongs to part
// 1 + (slot - 1) % (ETG_TU_PARTS - 1): that part instantiates the kernel, every other part (the host side included) only
// declares it.  The combinations are the ones dispatch16 / dispatch4 (etg_layout.h) can pick; a launch of a combination that
// is missing here fails at link time (undefined __device_stub__), not at run time.
#define ETG_ARGS_SETTLE KCfg, DevState, const uint8_t*
#define ETG_ARGS_FINISH KCfg, DevState, const uint8_t*, float*
#define ETG_ARGS_STEP KCfg, DevState, const float*, const uint8_t*, float*, float*, uint8_t*, float*
#define ETG_ARGS_STEP_AR KCfg, DevState, const float*, const uint8_t*, float*, float*, uint8_t*, float*, NextDyn, TermOut
#define ETG_ARGS_ROLLOUT KCfg, DevState, int, float*, StatOut
#define ETG_ARGS_TAPE KCfg, DevState, int, const float*, float*, TapeOut
#define ETG_ARGS_POLICY KCfg, DevState, PolicyW, int, float, float*
#define ETG_ARGS_POLICY_REC KCfg, DevState, PolicyW, int, float, float*, RecOut
#define ETG_ARGS_STEP_POLICY KCfg, DevState, PolicyW, float, float*, StepPolOut
#define ETG_ARGS_STEP_POLICY_AR KCfg, DevState, PolicyW, float, float*, StepPolOut, NextDyn
#define ETG_ARGS_COLLECT KCfg, DevState, PolicyW, float, float*, CollectOut, int, int
#define ETG_ARGS_STEP_POLICY_SCAN KCfg, DevState, PolicyW, float, float*, StepPolOut, ScanPol
#define ETG_ARGS_STEP_POLICY_SCAN_AR KCfg, DevState, PolicyW, float, float*, StepPolOut, NextDyn, ScanPol
#define ETG_ARGS_COLLECT_SCAN KCfg, DevState, PolicyW, float, float*, CollectOut, int, int, ScanPol
#if ETG_TU_PARTS > 1
#define ETG_SLOT_OWNER(S) (1 + ((S) - 1) % (ETG_TU_PARTS - 1))
#if ETG_SLOT_OWNER(1) == ETG_TU_PART
#define ETG_TPL_1 template
#else
#define ETG_TPL_1 extern template
#endif
#if ETG_SLOT_OWNER(2) == ETG_TU_PART
#define ETG_TPL_2 template
#else
#define ETG_TPL_2 extern template
#endif
#if ETG_SLOT_OWNER(3) == ETG_TU_PART
#define ETG_TPL_3 template
#else
#define ETG_TPL_3 extern template
#endif
#if ETG_SLOT_OWNER(4) == ETG_TU_PART
#define ETG_TPL_4 template
#else
#define ETG_TPL_4 extern template
#endif
#if ETG_SLOT_OWNER(5) == ETG_TU_PART
#define ETG_TPL_5 template
#else
#define ETG_TPL_5 extern template
#endif
#if ETG_SLOT_OWNER(6) == ETG_TU_PART
#define ETG_TPL_6 template
#else
#define ETG_TPL_6 extern template
#endif
#if ETG_SLOT_OWNER(7) == ETG_TU_PART
#define ETG_TPL_7 template
#else
#define ETG_TPL_7 extern template
#endif
// Slots 8..10 belong to parts ETG_TU_PARTS .. ETG_TU_PARTS + 2, which hold nothing else: the closed-loop kernels with SCAN
// (ETG_SCAN_INST16 below).  In a part of their neighbours they would add callers of the heightfield functions to its module, and
// the compiler then schedules that part's non-FLAT tick kernels differently (seen in 4 of them, k_rollout16 among them) -- the
// existing kernels are to stay the instruction streams they are.
#if ETG_TU_PARTS == ETG_TU_PART
#define ETG_TPL_8 template
#else
#define ETG_TPL_8 extern template
#endif
#if ETG_TU_PARTS + 1 == ETG_TU_PART
#define ETG_TPL_9 template
#else
#define ETG_TPL_9 extern template
#endif
#if ETG_TU_PARTS + 2 == ETG_TU_PART
#define ETG_TPL_10 template
#else
#define ETG_TPL_10 extern template
#endif
// 16-lane families: <FLAT, KNEE, PLAIN> in the order of ETG_VARIANTS16 (etg_layout.h)
#define ETG_INST16(KERN, S0, S1, S2, S3, S4, S5, ...)                          \
  ETG_TPL_##S0 __global__ void KERN<true, true, true>(__VA_ARGS__);            \
  ETG_TPL_##S1 __global__ void KERN<true, false, true>(__VA_ARGS__);           \
  ETG_TPL_##S2 __global__ void KERN<true, true, false>(__VA_ARGS__);           \
  ETG_TPL_##S3 __global__ void KERN<false, true, true>(__VA_ARGS__);           \
  ETG_TPL_##S4 __global__ void KERN<false, false, true>(__VA_ARGS__);          \
  ETG_TPL_##S5 __global__ void KERN<false, true, false>(__VA_ARGS__);
// the same six variants for the SCAN kernels, in a table of their own: their slots are the parts of their own (above), and the
// variant x entry-point matrix of the physics parity suite (tests/variant_matrix.py), which reads the ETG_INST* rows, has no
// cell for them -- the scan kernels run the tick code of k_step_policy16* / k_collect_policy16, whose cells it has
#define ETG_SCAN_INST16(KERN, S0, S1, S2, S3, S4, S5, ...)                     \
  ETG_TPL_##S0 __global__ void KERN<true, true, true>(__VA_ARGS__);            \
  ETG_TPL_##S1 __global__ void KERN<true, false, true>(__VA_ARGS__);           \
  ETG_TPL_##S2 __global__ void KERN<true, true, false>(__VA_ARGS__);           \
  ETG_TPL_##S3 __global__ void KERN<false, true, true>(__VA_ARGS__);           \
  ETG_TPL_##S4 __global__ void KERN<false, false, true>(__VA_ARGS__);          \
  ETG_TPL_##S5 __global__ void KERN<false, true, false>(__VA_ARGS__);
// 4-lane families: <FLAT, PLAIN, BODY> in the order of ETG_VARIANTS4 (etg_layout.h)
#define ETG_INST4(KERN, S0, S1, S2, S3, S4, S5, S6, S7, ...)                   \
  ETG_TPL_##S0 __global__ void KERN<true, false, 3>(__VA_ARGS__);              \
  ETG_TPL_##S1 __global__ void KERN<false, false, 3>(__VA_ARGS__);             \
  ETG_TPL_##S2 __global__ void KERN<true, false, 1>(__VA_ARGS__);              \
  ETG_TPL_##S3 __global__ void KERN<false, false, 1>(__VA_ARGS__);             \
  ETG_TPL_##S4 __global__ void KERN<true, true, 0>(__VA_ARGS__);               \
  ETG_TPL_##S5 __global__ void KERN<true, false, 0>(__VA_ARGS__);              \
  ETG_TPL_##S6 __global__ void KERN<false, true, 0>(__VA_ARGS__);              \
  ETG_TPL_##S7 __global__ void KERN<false, false, 0>(__VA_ARGS__);
// closed-loop 4-lane family: <FLAT, BF16, PLAIN, BODY> in the order of ETG_VARIANTS4 without BODY == 3 (etg_rollout_policy refuses it)
#define ETG_INSTP4(KERN, BF, S0, S1, S2, S3, S4, S5, ...)                      \
  ETG_TPL_##S0 __global__ void KERN<true, BF, false, 1>(__VA_ARGS__);          \
  ETG_TPL_##S1 __global__ void KERN<false, BF, false, 1>(__VA_ARGS__);         \
  ETG_TPL_##S2 __global__ void KERN<true, BF, true, 0>(__VA_ARGS__);           \
  ETG_TPL_##S3 __global__ void KERN<true, BF, false, 0>(__VA_ARGS__);          \
  ETG_TPL_##S4 __global__ void KERN<false, BF, true, 0>(__VA_ARGS__);          \
  ETG_TPL_##S5 __global__ void KERN<false, BF, false, 0>(__VA_ARGS__);
ETG_INST16(k_settle16, 1, 2, 3, 4, 5, 6, ETG_ARGS_SETTLE)
ETG_INST16(k_finish16, 7, 1, 2, 3, 4, 5, ETG_ARGS_FINISH)
ETG_INST16(k_step16, 6, 7, 1, 2, 3, 4, ETG_ARGS_STEP)
ETG_INST16(k_step16_ar, 5, 6, 7, 1, 2, 3, ETG_ARGS_STEP_AR)
ETG_INST16(k_rollout16, 4, 5, 6, 7, 1, 2, ETG_ARGS_ROLLOUT)
ETG_INST16(k_rollout_actions16, 3, 4, 5, 6, 7, 1, ETG_ARGS_TAPE)
ETG_INST16(k_rollout_policy16w, 2, 4, 6, 1, 3, 5, ETG_ARGS_POLICY)
ETG_INST16(k_rollout_policy16w_rec, 7, 2, 4, 6, 1, 3, ETG_ARGS_POLICY_REC)
ETG_INST16(k_step_policy16, 3, 5, 7, 2, 4, 6, ETG_ARGS_STEP_POLICY)
ETG_INST16(k_step_policy16_ar, 6, 1, 3, 5, 7, 2, ETG_ARGS_STEP_POLICY_AR)
ETG_INST16(k_collect_policy16, 4, 6, 1, 3, 5, 7, ETG_ARGS_COLLECT)
ETG_INST16(k_rollout_policy16, 1, 2, 3, 4, 5, 6, ETG_ARGS_POLICY)
ETG_INST16(k_rollout_policy16_rec, 6, 7, 1, 2, 3, 4, ETG_ARGS_POLICY_REC)
ETG_INST4(k_settle, 5, 6, 7, 1, 2, 3, 4, 5, ETG_ARGS_SETTLE)
ETG_INST4(k_finish, 6, 7, 1, 2, 3, 4, 5, 6, ETG_ARGS_FINISH)
ETG_INST4(k_step, 7, 1, 2, 3, 4, 5, 6, 7, ETG_ARGS_STEP)
ETG_INST4(k_step_ar, 1, 2, 3, 4, 5, 6, 7, 1, ETG_ARGS_STEP_AR)
ETG_INST4(k_rollout, 2, 3, 4, 5, 6, 7, 1, 2, ETG_ARGS_ROLLOUT)
ETG_INST4(k_rollout_actions, 3, 4, 5, 6, 7, 1, 2, 3, ETG_ARGS_TAPE)
ETG_INSTP4(k_rollout_policy4, false, 4, 5, 6, 7, 1, 2, ETG_ARGS_POLICY)
ETG_INSTP4(k_rollout_policy4, true, 3, 4, 5, 6, 7, 1, ETG_ARGS_POLICY)
ETG_SCAN_INST16(k_step_policy16_scan, 8, 9, 10, 8, 9, 10, ETG_ARGS_STEP_POLICY_SCAN)
ETG_SCAN_INST16(k_step_policy16_scan_ar, 9, 10, 8, 9, 10, 8, ETG_ARGS_STEP_POLICY_SCAN_AR)
ETG_SCAN_INST16(k_collect_policy16_scan, 10, 8, 9, 10, 8, 9, ETG_ARGS_COLLECT_SCAN)
#endif   // ETG_TU_PARTS > 1

}  // namespace etg

#if ETG_TU_HOST
#include "render_core.h"
#include "../../include/etgsim_render.h"
#include "snapshot_core.h"
#include "../../include/etgsim_snapshot.h"
#include "scan_core.h"
#include "../../include/etgsim_heightscan.h"
#include "dev_buffers.h"
#include <string.h>

// ====================================================================== C ABI
using namespace etg;

struct EtgHandle {   // etg_create's `new EtgHandle()` zeroes the members without an initialiser (K, M, D, NX: every pointer null)
  int device = 0, N = 0;
  KCfg K;
  ModelF M;
  DevState D;
  float* hf = nullptr;
  int lanes = 0;                      // 4 or 16 lanes per robot (EtgConfig.lanes_per_robot)
  unsigned long long push_calls = 0;  // stream position of etg_random_pushes
  unsigned obs_calls = 0;             // stream position of the sensor noise: observations written so far
  bool was_reset = false;             // etg_step before the first etg_reset is a caller error (state undefined)
  bool fext_set = false, push_on = false;   // a set force / random pushes are installed: K.ext_force = fext_set || push_on
  bool all_cached = false;            // every robot has a valid cached settle (true after a full etg_reset until parameters,
                                      // terrain or -- on a heightfield -- start offsets change): etg_step_autoreset's fast path
  // etg_rollout_wave_cycles: [launches of the last open-loop rollout][wavefronts] shader-clock cycles, written by the launches
  long long* wave_cycles = nullptr;
  int wc_cap = 0, wc_launches = 0, wc_waves = 0;
  int rollout_chunk = 400;      // control steps per fused launch (400: one launch for BASELINE's episode, ~37 ms: fewer launches = fewer chip-wide barriers, 93.3 us per step against 94.0 at 50; 25 .. 400 measured, profiles/r06_chunk_sweep.txt; ETG_ROLLOUT_CHUNK overrides it: a measurement aid)
  float *tmp_obs = nullptr, *tmp_reward = nullptr;  // sinks for etg_rollout_openloop
  uint8_t* tmp_done = nullptr;
  // etg_prepare_next_dynamics: rows waiting for the robots' next episodes + the scratch state / ring / flags its settle runs on
  NextDyn NX;
  float *nx_base = nullptr, *nx_leg = nullptr, *nx_ring = nullptr;
  unsigned char* nx_cache_ok = nullptr;
  uint8_t* nx_mask = nullptr;   // etg_prepare_next_dynamics: the call's mask without the robots whose episode is younger than the ring
  // all_cached again after MASKED resets: every invalidation bumps inval_seq; a masked etg_reset ends with a count of the robots
  // still without a cached settle, written with the sequence number it ran under to pinned host memory (cached_report[0] = count,
  // [1] = seq); the next etg_step_autoreset / etg_prepare_next_dynamics trusts a zero count only under the CURRENT number
  unsigned inval_seq = 1;
  volatile unsigned* cached_report = nullptr;   // pinned host memory, also mapped on the device (cached_report_dev)
  unsigned* cached_report_dev = nullptr;
  // etg_render: lowest / highest height of the heightfield, taken at the first render after etg_set_heightfield
  bool hf_range_ok = false;
  float hf_lo = 0.0f, hf_hi = 0.0f;
};

// ---- the handle's per-robot device arrays, ONE row each, for everything that has to know them all: etg_create allocates the
// CORE group, ensure_next_arrays the NEXT group (on first use), etg_destroy frees every row, snapshot_table takes the RECORD rows,
// in this order, as the segments of a snapshot record -- so the order of those rows is part of the record format.  The shape is
// snapshot_core.h's and gives the size too: rows * per * N words, or N bytes.  SCRATCH, in no record: tmp_* (sinks of
// etg_rollout_openloop), nx_base .. nx_mask (the prepared settle's state, dead when etg_prepare_next_dynamics returns).  Not in
// the table, freed by etg_destroy: hf (sized by the heightfield), wave_cycles (per rollout call), cached_report (pinned host memory).
enum ArrayGroup { CORE = 1, NEXT = 2 };
enum ArrayUse { SCRATCH, RECORD };
struct HandleArray {
  size_t slot;   // where the handle keeps the pointer: its offset in EtgHandle
  int rows, per;
  bool bytes;    // the slot points at one-byte elements, a flag array (rows = per = 1)
  ArrayGroup group; ArrayUse use;
};
#define ARR(m, rows, per, group, use) HandleArray{offsetof(EtgHandle, m), rows, per, sizeof(*((EtgHandle*)nullptr)->m) == 1, group, use}
static constexpr HandleArray kHandleArrays[] = {
    ARR(D.base, BS_N, 1, CORE, RECORD),       ARR(D.leg, LG_N, 4, CORE, RECORD),       ARR(D.ctl, CT_N, 1, CORE, RECORD),
    ARR(D.ictl, IC_N, 1, CORE, RECORD),       ARR(D.legctl, LC_N, 4, CORE, RECORD),    ARR(D.etgp, EP_N, 1, CORE, RECORD),
    ARR(D.par, PR_N, 4, CORE, RECORD),        ARR(D.ring, RING * 8, 4, CORE, RECORD),  ARR(D.dyn, 1, ETG_DYN_DIM, CORE, RECORD),
    ARR(D.cache_base, BS_N, 1, CORE, RECORD), ARR(D.cache_leg, LG_N, 4, CORE, RECORD), ARR(D.cache_ring, RING * 8, 4, CORE, RECORD),
    ARR(D.cache_ok, 1, 1, CORE, RECORD),      ARR(D.reset_off, 2, 1, CORE, RECORD),    ARR(D.cache_off, FIN_ROWS, 1, CORE, RECORD),
    ARR(tmp_obs, 1, ETG_OBS_DIM, CORE, SCRATCH), ARR(tmp_reward, 1, 1, CORE, SCRATCH), ARR(tmp_done, 1, 1, CORE, SCRATCH),
    ARR(NX.par, PR_N, 4, NEXT, RECORD),       ARR(NX.dyn, 1, ETG_DYN_DIM, NEXT, RECORD), ARR(NX.ok, 1, 1, NEXT, RECORD),
    ARR(nx_base, BS_N, 1, NEXT, SCRATCH),     ARR(nx_leg, LG_N, 4, NEXT, SCRATCH),     ARR(nx_ring, RING * 8, 4, NEXT, SCRATCH),
    ARR(nx_cache_ok, 1, 1, NEXT, SCRATCH),    ARR(nx_mask, 1, 1, NEXT, SCRATCH)};   // (nx_mask last: ensure_next_arrays)
#undef ARR
static_assert([] { int n = 0; for (const HandleArray& a : kHandleArrays) n += a.use == RECORD; return n; }() <= snapshot::kMaxSegs,
              "snapshot::Table is too small for the RECORD rows");
static void** array_slot(EtgHandle* h, const HandleArray& a) { return (void**)((char*)h + a.slot); }
static std::vector<dev::Buf> array_bufs(EtgHandle* h, int groups) {   // the rows of the given groups as buffers, sized by their shapes
  std::vector<dev::Buf> bufs;
  for (const HandleArray& a : kHandleArrays)
    if (a.group & groups) bufs.push_back({array_slot(h, a), a.bytes ? (size_t)h->N : (size_t)a.rows * a.per * h->N * 4});
  return bufs;
}

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(ETG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

extern "C" const char* etg_last_error(void) { return g_err.c_str(); }
// shared with policy_mlp.hip so that one etg_last_error() serves the whole ABI
extern "C" void etg_set_last_error_(const char* msg) { g_err = msg ? msg : ""; }
extern "C" int etg_lanes_per_robot(const EtgHandle* h) { return h ? h->lanes : ETG_ERR_BAD_ARG; }
int etg_version(void) { return 2; }
int etg_config_size(void) { return (int)sizeof(EtgConfig); }
int etg_model_size(void) { return (int)sizeof(EtgRobotModel); }

static int grid_for(const EtgHandle* h) { return (4 * h->N + BLOCK - 1) / BLOCK; }

extern "C" int etg_create(const EtgConfig* cfg, const EtgRobotModel* model, int device, EtgHandle** out) {
  if (!cfg || !model || !out) return fail(ETG_ERR_BAD_ARG, "etg_create: null argument");
  if (cfg->num_envs <= 0 || cfg->num_envs > (1 << 20)) return fail(ETG_ERR_BAD_ARG, "etg_create: num_envs must be in 1..1048576");
  if (cfg->action_repeat <= 0 || cfg->sim_dt <= 0) return fail(ETG_ERR_BAD_ARG, "etg_create: bad action_repeat/sim_dt");
  // the rest of the configuration is checked before a device is touched, so a bad one reads the same on any box
  if (cfg->solver_iters <= 0 || cfg->solver_iters > 1000) return fail(ETG_ERR_BAD_ARG, "etg_create: solver_iters must be in 1..1000");
  if (!(cfg->solver_residual >= 0)) return fail(ETG_ERR_BAD_ARG, "etg_create: solver_residual must be >= 0 (0 = a fixed number of sweeps)");
  if (cfg->friction_model != 0 && cfg->friction_model != 1) return fail(ETG_ERR_BAD_ARG, "etg_create: friction_model must be 0 (disc) or 1 (pyramid)");
  if (!(cfg->pd_latency >= 0)) return fail(ETG_ERR_BAD_ARG, "etg_create: pd_latency must be >= 0 seconds");
  // (beyond the ring depth the blend of minitaur.py:1185-1188 would extrapolate between aliased slots)
  if (cfg->pd_latency >= (etg::RING - 2) * cfg->sim_dt)
    return fail(ETG_ERR_BAD_ARG, "etg_create: pd_latency must be below (ring depth - 2) * sim_dt = 62 ticks");
  if (!(cfg->warmstart >= 0) || !(cfg->warmstart_friction >= 0)) return fail(ETG_ERR_BAD_ARG, "etg_create: warm-start factors must be >= 0");
  if (!(cfg->contact_slop >= 0)) return fail(ETG_ERR_BAD_ARG, "etg_create: contact_slop must be >= 0");
  if (!(cfg->foot_restitution >= 0) || cfg->foot_restitution > 1) return fail(ETG_ERR_BAD_ARG, "etg_create: foot_restitution must be in [0, 1]");
  if (cfg->settle_ticks < 0) return fail(ETG_ERR_BAD_ARG, "etg_create: settle_ticks must not be negative");
  if (cfg->motor_mode < 0 || cfg->motor_mode > 2) return fail(ETG_ERR_BAD_ARG, "etg_create: motor_mode must be 0 (POSITION), 1 (TORQUE) or 2 (HYBRID)");
  if (cfg->body_contacts < 0 || cfg->body_contacts > 3) return fail(ETG_ERR_BAD_ARG, "etg_create: body_contacts must be 0, 1, 2 or 3");
  if (!(cfg->body_friction >= 0.0)) return fail(ETG_ERR_BAD_ARG, "etg_create: body_friction must be >= 0");
  if (cfg->body_contacts == 3 && cfg->lanes_per_robot == 16)
    return fail(ETG_ERR_BAD_ARG, "etg_create: body_contacts = 3 (three body rows per leg) needs the 4-lanes-per-robot mapping");
  if (cfg->terrain != 0 && cfg->terrain != 1) return fail(ETG_ERR_BAD_ARG, "etg_create: terrain must be 0 (plane) or 1 (heightfield)");
  if (cfg->terrain == 1 && (cfg->hf_nx < 2 || cfg->hf_ny < 2 || !(cfg->hf_cell > 0) || cfg->hf_bands < 0 ||
                            (cfg->hf_bands > 1 && cfg->hf_ny % cfg->hf_bands != 0)))
    return fail(ETG_ERR_BAD_ARG, "etg_create: a heightfield needs hf_nx, hf_ny >= 2 (per band), hf_cell > 0 and hf_ny divisible by hf_bands");
  if (cfg->etg_dt <= 0 || cfg->etg_T <= 0) return fail(ETG_ERR_BAD_ARG, "etg_create: etg_dt and etg_T must be positive");
  if (cfg->joint_limits)
    for (int k = 0; k < 3; k++)
      if (!(cfg->joint_lower[k] < cfg->joint_upper[k])) return fail(ETG_ERR_BAD_ARG, "etg_create: joint_lower must be below joint_upper");
  if (cfg->lanes_per_robot != 0 && cfg->lanes_per_robot != 4 && cfg->lanes_per_robot != 16)
    return fail(ETG_ERR_BAD_ARG, "etg_create: lanes_per_robot must be 0 (auto), 4 or 16");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(ETG_ERR_NO_DEVICE, "etg_create: no HIP device (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(ETG_ERR_BAD_ARG, "etg_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  EtgHandle* h = new EtgHandle();
  h->device = device;
  h->N = cfg->num_envs;
  h->K = make_kcfg(*cfg, *model);
  h->M = make_modelf(*model);
  if (const char* e = getenv("ETG_ROLLOUT_CHUNK")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 100000) h->rollout_chunk = v;
  }
  // 0 = auto.  Both kernels hold one wave per SIMD (register footprint), so the chip runs 1024 waves
  // at a time: 16 lanes/robot fills it with 4096 robots and is faster per robot up to there; beyond
  // that the 4-lanes/robot kernel packs 4x the robots per wave (measured crossover).
  // auto: the 16-lane mapping while it fills the chip once (4096 robots = one wave per SIMD); with body rows (modes 1 / 2) up to
  // 8192 -- two rounds of the 16-lane kernel (45 M env-steps/s) still beat the half-filled 4-lane one, whose wave waits for the
  // slowest of SIXTEEN robots (36 M; profiles/r05_ab_experiments.txt section 8); above that the 4-lane mapping (16384: 72 M vs 41 M)
  const int auto16 = (cfg->body_contacts == 1 || cfg->body_contacts == 2) ? 8192 : 4096;
  h->lanes = cfg->lanes_per_robot != 0 ? cfg->lanes_per_robot : (cfg->num_envs <= auto16 ? 16 : 4);
  if (cfg->body_contacts == 3) h->lanes = 4;   // six rows per leg: the 16-lane mapping has one spare lane per leg
  float* ddyn = nullptr;   // the default parameter rows on their way to the device
  int rc = [&]() -> int {  // (HIP_TRY returns from here: whatever fails, the cleanup below runs)
    if (int r = dev::alloc(array_bufs(h, CORE), "etg_create")) return r;
    h->K.cring = h->D.cache_ring;
    // default physical parameters = param2dynamic_dict(zeros(48)) (train.py:112-126)
    std::vector<float> row(ETG_DYN_DIM, 1.0f);
    row[0] = 40.0f; row[1] = 0.2f; row[2] = 1.5f;
    for (int j = 0; j < 12; j++) { row[21 + j] = 80.0f; row[33 + j] = (j % 3 == 0) ? 1.0f : 2.0f; }
    row[45] = 0.0f; row[46] = 0.0f; row[47] = -10.0f;
    std::vector<float> dyn((size_t)h->N * ETG_DYN_DIM);
    for (size_t i = 0; i < dyn.size(); i++) dyn[i] = row[i % ETG_DYN_DIM];
    if (hipMalloc((void**)&ddyn, dyn.size() * 4) != hipSuccess) return fail(ETG_ERR_ALLOC, "etg_create: hipMalloc failed");
    HIP_TRY(hipMemcpy(ddyn, dyn.data(), dyn.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_set_params, dim3(grid_for(h)), dim3(BLOCK), 0, 0, h->K, h->M, h->D, ddyn, nullptr, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_set_strength, dim3((4 * h->N + 255) / 256), dim3(256), 0, 0, h->K, h->D, (const float*)nullptr, (const uint8_t*)nullptr);
    HIP_TRY(hipDeviceSynchronize());
    return ETG_OK;
  }();
  const hipError_t e = hipFree(ddyn);   // (null, a no-op, when the steps above did not get that far)
  if (!rc && e != hipSuccess) rc = fail(ETG_ERR_HIP, std::string("hipFree(ddyn): ") + hipGetErrorString(e));
  if (rc) { etg_destroy(h); return rc; }
  *out = h;
  return ETG_OK;
}

extern "C" void etg_destroy(EtgHandle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  dev::release(array_bufs(h, CORE | NEXT));
  if (h->hf) (void)hipFree(h->hf);
  if (h->wave_cycles) (void)hipFree(h->wave_cycles);
  if (h->cached_report) (void)hipHostFree((void*)h->cached_report);
  delete h;
}

// the next launch writes `n` observations per robot: give them the next n positions of the sensor-noise stream
static inline void advance_obs_stream(EtgHandle* h, int n) {
  h->K.noise_call = h->obs_calls;
  h->obs_calls += (unsigned)n;
}

// noise for the observation rows the launch before wrote last (stream position K.noise_call + n - 1)
static inline void launch_obs_noise(EtgHandle* h, int n, const uint8_t* mask, float* obs, hipStream_t s, int invert = 0, int back = 0) {
  if (!h->K.noise_on || !obs) return;   // back: stream positions before the newest one (the step's row when a reset row follows it)
  hipLaunchKernelGGL(k_add_noise, dim3((16 * h->N + 255) / 256), dim3(256), 0, s, h->K,
                     h->K.noise_call + (unsigned)(n - 1) - (unsigned)back, mask, invert, obs);
}

// noise for the rows a fused rollout launch of n steps left in `obs` (stream positions K.noise_call .. + n - 1)
static inline void launch_rollout_noise(EtgHandle* h, int n, float* obs, hipStream_t s) {
  if (!h->K.noise_on || !obs) return;
  if (!h->K.stop_at_done) { launch_obs_noise(h, n, nullptr, obs, s); return; }   // every row is the last step's
  hipLaunchKernelGGL(k_add_noise_rows, dim3((16 * h->N + 255) / 256), dim3(256), 0, s, h->K, h->D, h->K.noise_call, (unsigned)n, obs);
}

// A tick kernel is launched in the variant that dispatch16 / dispatch4 (etg_layout.h: the lists of the variants and the rules of
// the choice) pick for the handle's configuration.  These are macros only because a kernel template's name cannot be passed as a
// value; every combination a launch can name is in the instantiation table above, or the library does not link.
#define ETG_V(c) decltype(c)::value
#define LAUNCH16(KERN, grid, stream, ...)                                                                             \
  dispatch16(h->K, [&](auto f_, auto k_, auto p_) {                                                                   \
    hipLaunchKernelGGL((KERN<ETG_V(f_), ETG_V(k_), ETG_V(p_)>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);           \
  })
#define LAUNCH4(KERN, grid, stream, ...)                                                                              \
  dispatch4(h->K, [&](auto f_, auto p_, auto b_) {                                                                    \
    hipLaunchKernelGGL((KERN<ETG_V(f_), ETG_V(p_), ETG_V(b_)>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);           \
  })
// the 16-lane kernel or its 4-lane counterpart; tick_grid(h): the mapping's grid for the whole batch
static dim3 tick_grid(const EtgHandle* h) { return dim3(h->lanes == 16 ? (h->N + 3) / 4 : grid_for(h)); }
#define LAUNCH_TICK(KERN16, KERN4, grid, stream, ...)                                                                 \
  do {                                                                                                                \
    if (h->lanes == 16) LAUNCH16(KERN16, grid, stream, __VA_ARGS__);                                                  \
    else LAUNCH4(KERN4, grid, stream, __VA_ARGS__);                                                                   \
  } while (0)

#define CHECK_HANDLE(h)                                         \
  if (!(h)) return fail(ETG_ERR_BAD_ARG, "null handle");       \
  HIP_TRY(hipSetDevice((h)->device));

extern "C" int etg_set_params(EtgHandle* h, const float* dyn, const float* etg_w, const float* etg_b, int per_env,
                              const uint8_t* mask, void* stream) {
  CHECK_HANDLE(h);
  if ((etg_w == nullptr) != (etg_b == nullptr)) return fail(ETG_ERR_BAD_ARG, "etg_set_params: pass both etg_w and etg_b or neither");
  if (dyn) { h->all_cached = false; h->inval_seq++; }   // the settle depends on the dynamic parameters
  if (dyn && h->NX.ok)              // (and rows prepared for the masked robots' next episodes came with a settle of their own)
    hipLaunchKernelGGL(k_next_flags, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->NX.ok, mask, (unsigned char)0);
  hipLaunchKernelGGL(k_fin_clear, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, mask);   // cached restarts: stale
  hipLaunchKernelGGL(k_set_params, dim3(grid_for(h)), dim3(BLOCK), 0, (hipStream_t)stream, h->K, h->M, h->D, dyn, etg_w,
                     etg_b, per_env, mask);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_set_heightfield(EtgHandle* h, const float* heights, void* stream) {
  CHECK_HANDLE(h);
  if (h->K.terrain != 1 || h->K.hf_nx < 2 || h->K.hf_ny < 2) return fail(ETG_ERR_STATE, "etg_set_heightfield: config has no heightfield");
  size_t bytes = (size_t)h->K.hf_nx * h->K.hf_ny * h->K.hf_bands * 4;
  if (!h->hf && hipMalloc((void**)&h->hf, bytes) != hipSuccess) return fail(ETG_ERR_ALLOC, "etg_set_heightfield: hipMalloc failed");
  HIP_TRY(hipMemcpyAsync(h->hf, heights, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(h->D.cache_ok, 0, h->N, (hipStream_t)stream));   // the settle depends on the terrain
  HIP_TRY(hipMemsetAsync(h->D.cache_off + (size_t)FIN_OK * h->N, 0, (size_t)h->N * 4, (hipStream_t)stream));
  h->all_cached = false;
  h->inval_seq++;
  h->K.hf = h->hf;
  h->hf_range_ok = false;
  return ETG_OK;
}

extern "C" int etg_set_external_force(EtgHandle* h, const float* force, void* stream) {
  CHECK_HANDLE(h);
  float* dst = h->D.ctl + (size_t)CT_FEXT * h->N;      // ctl[CT_FEXT + k][N]
  if (!force) {
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)3 * h->N * 4, (hipStream_t)stream));
    h->fext_set = false;
    h->K.ext_force = h->push_on;     // pending random pushes keep acting
    return ETG_OK;
  }
  hipLaunchKernelGGL(k_set_fext, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, force);
  HIP_TRY(hipGetLastError());
  h->fext_set = true;
  h->K.ext_force = 1;
  return ETG_OK;
}

extern "C" int etg_set_motor_strength(EtgHandle* h, const float* ratios, const uint8_t* mask, void* stream) {
  CHECK_HANDLE(h);
  hipLaunchKernelGGL(k_set_strength, dim3((4 * h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, ratios, mask);
  HIP_TRY(hipGetLastError());
  // ratios installed for anybody: the kernels with the robot-layer options read them (a later NULL for everybody switches back)
  h->K.strength_on = ratios ? 1 : (mask ? h->K.strength_on : 0);
  // the reset settle runs under the motor model too: cached settles of the touched robots are stale (k_set_strength cleared
  // their flags), and so are the settles prepared for their next episodes
  h->all_cached = false;
  h->inval_seq++;
  if (h->NX.ok)
    hipLaunchKernelGGL(k_next_flags, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->NX.ok, mask, (unsigned char)0);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_random_pushes(EtgHandle* h, uint64_t seed, float prob, int duration_steps, float fmin, float fmax,
                                 void* stream) {
  CHECK_HANDLE(h);
  if (prob < 0.0f || duration_steps < 1 || fmax < fmin) return fail(ETG_ERR_BAD_ARG, "etg_random_pushes: bad arguments");
  hipLaunchKernelGGL(k_random_pushes, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D,
                     (unsigned long long)seed, h->push_calls++, prob, duration_steps, fmin, fmax);
  HIP_TRY(hipGetLastError());
  h->push_on = true;
  h->K.ext_force = 1;
  return ETG_OK;
}

extern "C" int etg_clear_pushes(EtgHandle* h, const uint8_t* mask, void* stream) {
  CHECK_HANDLE(h);
  hipLaunchKernelGGL(k_clear_pushes, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, mask);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// ---- parameters for the NEXT episode (etg_prepare_next_dynamics)
// robots without a valid cached settle, counted after a masked reset (one workgroup; see EtgHandle::cached_report)
#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void __launch_bounds__(256) k_count_uncached(KCfg K, DevState D, unsigned seq, unsigned* report) {
  __shared__ unsigned part[256];
  unsigned n = 0;
  for (int env = threadIdx.x; env < K.n_env; env += 256) n += D.cache_ok[env] ? 0u : 1u;
  part[threadIdx.x] = n;
  __syncthreads();
  for (unsigned s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&report[0], part[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(&report[1], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
#endif
// host side: has a masked reset, run under the current invalidation number, reported that every robot is cached again?
static inline void refresh_all_cached(EtgHandle* h) {
  if (h->all_cached || !h->cached_report) return;
  const unsigned seq = h->cached_report[1];
  __sync_synchronize();
  if (seq == h->inval_seq && h->cached_report[0] == 0u) h->all_cached = true;
}

// the NEXT group, allocated and zeroed on the caller's stream on first use (nx_mask, its last row, is null until all of it is there)
static int ensure_next_arrays(EtgHandle* h, const char* who, hipStream_t s) {
  return h->nx_mask ? ETG_OK : dev::alloc(array_bufs(h, NEXT), who, &s);
}

extern "C" int etg_prepare_next_dynamics(EtgHandle* h, const float* dyn, const uint8_t* mask, void* stream) {
  CHECK_HANDLE(h);
  if (!dyn) return fail(ETG_ERR_BAD_ARG, "etg_prepare_next_dynamics: dyn is null");
  refresh_all_cached(h);
  if (!h->was_reset || !h->all_cached)
    return fail(ETG_ERR_STATE, "etg_prepare_next_dynamics: every robot needs a valid cached settle (a full etg_reset, or masked resets "
                               "that covered every robot whose parameters, terrain or start offset changed)");
  const size_t NL = 4 * (size_t)h->N;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = ensure_next_arrays(h, "etg_prepare_next_dynamics", s)) return rc;
  const dim3 ge((h->N + 255) / 256), gc((4 * h->N + 255) / 256);
  // a view of the robot arrays whose parameters are the NEXT rows, whose live state / ring are scratch (the robots keep running
  // on theirs) and whose settle cache is the real one: k_settle* leaves the settled state of the new rows in the cache
  DevState Dn = h->D;
  Dn.par = h->NX.par;
  Dn.dyn = h->NX.dyn;
  Dn.base = h->nx_base; Dn.leg = h->nx_leg; Dn.ring = h->nx_ring;
  Dn.cache_ok = h->nx_cache_ok;
  // the motor strength ratios are not derived from the dynamic_param row: the scratch settle runs under the robots' own
  // (found by the round-4 soak run: zeros there left the robot limp during the prepared settle whenever a non-plain kernel ran it)
  HIP_TRY(hipMemcpyAsync(h->NX.par + (size_t)PR_STR * NL, h->D.par + (size_t)PR_STR * NL, (size_t)(PR_N - PR_STR) * NL * 4, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_next_old_enough, ge, dim3(256), 0, s, h->K, h->D, mask, h->nx_mask);
  mask = h->nx_mask;   // robots in the first RING ticks of their episode still read the cache's ring: not this time
  hipLaunchKernelGGL(k_set_params, dim3(grid_for(h)), dim3(BLOCK), 0, s, h->K, h->M, Dn, dyn, (const float*)nullptr,
                     (const float*)nullptr, 0, mask);   // (derives the rows; clears the scratch "cached" flag of the masked robots)
  LAUNCH_TICK(k_settle16, k_settle, tick_grid(h), s, h->K, Dn, mask);
  hipLaunchKernelGGL(k_cache_sync, gc, dim3(256), 0, s, h->K, Dn, mask);      // scratch ring -> the cache's ring
  hipLaunchKernelGGL(k_fin_clear, ge, dim3(256), 0, s, h->K, h->D, mask);     // cached first observations: stale
  hipLaunchKernelGGL(k_next_flags, ge, dim3(256), 0, s, h->K, h->NX.ok, mask, (unsigned char)1);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_next_dynamics_pending(EtgHandle* h, uint8_t* pending, void* stream) {
  CHECK_HANDLE(h);
  if (!pending) return fail(ETG_ERR_BAD_ARG, "etg_next_dynamics_pending: pending is null");
  if (!h->NX.ok) { HIP_TRY(hipMemsetAsync(pending, 0, h->N, (hipStream_t)stream)); return ETG_OK; }
  HIP_TRY(hipMemcpyAsync(pending, h->NX.ok, h->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return ETG_OK;
}

extern "C" int etg_reset(EtgHandle* h, const uint8_t* mask, float* obs, void* stream) {
  CHECK_HANDLE(h);
  if (!obs) return fail(ETG_ERR_BAD_ARG, "etg_reset: obs is null");
  if (h->K.terrain == 1 && !h->K.hf) return fail(ETG_ERR_STATE, "etg_reset: heightfield not set");
  h->was_reset = true;
  advance_obs_stream(h, 1);
  if (h->NX.ok) {   // rows prepared for the next episode of the masked robots: this reset starts it
    hipLaunchKernelGGL(k_next_take, dim3((4 * h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, h->NX, mask);
    hipLaunchKernelGGL(k_next_flags, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->NX.ok, mask, (unsigned char)0);
  }
  // 1. settle the masked robots that have no valid settle cache (kernel exits at once for the others)
  // 2. snapshot their ring / restore state + ring of the cached ones, mark everything masked as cached
  // 3. the part after the settle: control state, episode accumulators, first observation
  const dim3 gc((4 * h->N + 255) / 256), ge((h->N + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  LAUNCH_TICK(k_settle16, k_settle, tick_grid(h), s, h->K, h->D, mask);
  hipLaunchKernelGGL(k_cache_sync, gc, dim3(256), 0, s, h->K, h->D, mask);
  hipLaunchKernelGGL(k_cache_mark, ge, dim3(256), 0, s, h->K, h->D, mask);
  LAUNCH_TICK(k_finish16, k_finish, tick_grid(h), s, h->K, h->D, mask, obs);
  hipLaunchKernelGGL(k_fin_store, ge, dim3(256), 0, s, h->K, h->D, mask, (const float*)obs);   // the clean row: before the noise
  launch_obs_noise(h, 1, mask, obs, s);
  if (mask && !h->all_cached) {   // did this masked reset settle the last robots without a cache?  (answer read by a later call)
    if (!h->cached_report) {
      void* p = nullptr;
      if (hipHostMalloc(&p, 2 * sizeof(unsigned), hipHostMallocMapped) == hipSuccess) {
        h->cached_report = (volatile unsigned*)p;
        h->cached_report[0] = 1u; h->cached_report[1] = 0u;
        if (hipHostGetDevicePointer((void**)&h->cached_report_dev, p, 0) != hipSuccess) {
          (void)hipHostFree(p);
          h->cached_report = nullptr;
        }
      }
    }
    if (h->cached_report) hipLaunchKernelGGL(k_count_uncached, dim3(1), dim3(256), 0, s, h->K, h->D, h->inval_seq, h->cached_report_dev);
  }
  HIP_TRY(hipGetLastError());
  if (!mask) h->all_cached = true;
  return ETG_OK;
}

#if ETG_TU_HOST   // small kernels: compiled with the host side only (part 0)
__global__ void k_set_reset_offsets(KCfg K, DevState D, const float* xy, const uint8_t* mask) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= K.n_env || (mask && !mask[env])) return;
  D.reset_off[env] = xy ? xy[2 * env] : 0.0f;
  D.reset_off[K.n_env + env] = xy ? xy[2 * env + 1] : 0.0f;
}
#endif
extern "C" int etg_set_sensor_noise(EtgHandle* h, const float* stdev, uint64_t seed) {
  CHECK_HANDLE(h);
  h->K.noise_on = 0;
  for (int k = 0; k < 5; k++) {
    const float v = stdev ? stdev[k] : 0.0f;
    if (!(v >= 0.0f)) return fail(ETG_ERR_BAD_ARG, "etg_set_sensor_noise: standard deviations must be >= 0");
    h->K.noise_std[k] = v;
    if (v > 0.0f) h->K.noise_on = 1;
  }
  h->K.noise_seed = seed;
  return ETG_OK;
}
extern "C" int etg_set_reset_offsets(EtgHandle* h, const float* xy, const uint8_t* mask, void* stream) {
  CHECK_HANDLE(h);
  hipLaunchKernelGGL(k_set_reset_offsets, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, xy, mask);
  hipLaunchKernelGGL(k_fin_clear, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, mask);
  HIP_TRY(hipGetLastError());
  if (h->K.terrain != 0) { h->all_cached = false; h->inval_seq++; }   // a heightfield settle is only valid at the offset it ran at
  return ETG_OK;
}

static int step_checks(EtgHandle* h, const float* action, float* obs, float* reward, uint8_t* done) {
  if (!obs || !reward || !done) return fail(ETG_ERR_BAD_ARG, "etg_step: obs/reward/done must be non-null");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_step: call etg_reset first");
  if (h->K.motor_mode == 2 && !action) return fail(ETG_ERR_BAD_ARG, "etg_step: the HYBRID motor mode needs a [N,60] command");
  return ETG_OK;
}

extern "C" int etg_step(EtgHandle* h, const float* action, const uint8_t* donef, float* obs, float* reward,
                        uint8_t* done, float* info, void* stream) {
  CHECK_HANDLE(h);
  if (int rc = step_checks(h, action, obs, reward, done)) return rc;
  advance_obs_stream(h, 1);
  LAUNCH_TICK(k_step16, k_step, tick_grid(h), (hipStream_t)stream, h->K, h->D, action, donef, obs, reward, done, info);
  launch_obs_noise(h, 1, nullptr, obs, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// One control step of the sub-batch [env0, env0 + count) only -- every array is the WHOLE batch's ([N, ...], indexed by the
// robot's number as in etg_step), the other robots' rows and states are not touched.  Sub-batches are independent (a robot's
// step depends on its own state, parameters and action: tests/test_gpu_parity3.py::test_wave_neighbours_...), so G ranges
// enqueued on G streams let each sub-batch start its next step when ITS slowest wavefront has finished instead of the batch's
// (env.step(groups=G), rollout_policy(fused=False, groups=G): train.py:129-178's loop with one barrier per group).
extern "C" int etg_step_range(EtgHandle* h, int env0, int count, const float* action, const uint8_t* donef, float* obs,
                              float* reward, uint8_t* done, float* info, void* stream) {
  CHECK_HANDLE(h);
  if (int rc = step_checks(h, action, obs, reward, done)) return rc;
  const int per_block = h->lanes == 16 ? BLOCK / 16 : BLOCK / 4;
  if (env0 < 0 || count <= 0 || env0 + count > h->N || env0 % 16 != 0 || (count % 16 != 0 && env0 + count != h->N))
    return fail(ETG_ERR_BAD_ARG, "etg_step_range: env0 and count must be multiples of 16 robots (the last range may end at N)");
  // the sensor-noise stream moves on with the range that starts at robot 0: the ranges of one control step are called in
  // ascending order and share the position, so that every robot draws what it draws in etg_step
  if (env0 == 0) advance_obs_stream(h, 1);
  KCfg K = h->K;
  K.block0 = env0 / per_block;
  const dim3 grid((count + per_block - 1) / per_block);
  LAUNCH_TICK(k_step16, k_step, grid, (hipStream_t)stream, K, h->D, action, donef, obs, reward, done, info);
  if (h->K.noise_on)
    hipLaunchKernelGGL(k_add_noise_range, dim3((16 * count + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->K.noise_call, env0, count, obs);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// etg_step_autoreset, and with T.obs its terminal rows (etg_step_autoreset_terminal): T changes nothing else the call writes
static int step_autoreset(EtgHandle* h, const float* action, const uint8_t* donef, float* obs, float* reward, uint8_t* done,
                          float* info, TermOut T, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  refresh_all_cached(h);
  if (!h->all_cached) {   // some robot needs a simulated settle: step, then the general reset path masked by the done bytes
    int rc = etg_step(h, action, donef, obs, reward, done, info, stream);
    if (rc != ETG_OK) return rc;
    if (T.obs) {          // the terminal rows are the step's rows (and their noise) as they stand before the reset
      HIP_TRY(hipMemcpyAsync(T.obs, obs, (size_t)h->N * ETG_OBS_DIM * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (T.ctx) hipLaunchKernelGGL(k_term_ctx, dim3((16 * h->N + 255) / 256), dim3(256), 0, s, h->K, h->D, done, T.ctx);
      HIP_TRY(hipGetLastError());
    }
    if (h->push_on && (rc = etg_clear_pushes(h, done, stream)) != ETG_OK) return rc;
    return etg_reset(h, done, obs, stream);
  }
  // every robot has a cached settle: step and restart in ONE launch (k_step16_ar / k_step_ar)
  if (int rc = step_checks(h, action, obs, reward, done)) return rc;
  advance_obs_stream(h, 2);                     // two rows per robot at most: the step's (position c) and the reset's (c + 1)
  LAUNCH_TICK(k_step16_ar, k_step_ar, tick_grid(h), s, h->K, h->D, action, donef, obs, reward, done, info, h->NX, T);
  launch_obs_noise(h, 2, nullptr, T.obs, s, 0, /*back=*/1);         // the terminal rows: every robot's step row (position c)
  if (T.obs && h->lanes != 16) {   // (4 lanes: the step's rows went to T.obs only; those of the robots that go on move to obs)
    hipLaunchKernelGGL(k_term_rows, dim3((h->N * ETG_OBS_DIM + 255) / 256), dim3(256), 0, s, h->K, T.obs, done, obs);
  } else {
    launch_obs_noise(h, 2, done, obs, s, /*invert=*/1, /*back=*/1);   // the step's rows of the robots that go on
  }
  launch_obs_noise(h, 2, done, obs, s);                            // the reset rows
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_step_autoreset(EtgHandle* h, const float* action, const uint8_t* donef, float* obs, float* reward,
                                  uint8_t* done, float* info, void* stream) {
  CHECK_HANDLE(h);
  return step_autoreset(h, action, donef, obs, reward, done, info, TermOut{nullptr, nullptr}, stream);
}

// etg_step_autoreset that keeps every robot's step observation before any restart (include/etgsim_terminal.h)
extern "C" int etg_step_autoreset_terminal(EtgHandle* h, const float* action, const uint8_t* donef, float* obs, float* terminal_obs,
                                           float* terminal_ctx, float* reward, uint8_t* done, float* info, void* stream) {
  CHECK_HANDLE(h);
  if (!terminal_obs) return fail(ETG_ERR_BAD_ARG, "etg_step_autoreset_terminal: terminal_obs must be non-null");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_step_autoreset_terminal: call etg_reset first");
  return step_autoreset(h, action, donef, obs, reward, done, info, TermOut{terminal_obs, terminal_ctx}, stream);
}

#ifdef ETG_TRACE_TICKS
extern "C" int etg_debug_set_trace(EtgHandle* h, float* buf) { if (!h) return ETG_ERR_BAD_ARG; h->K.trace = buf; return ETG_OK; }
#endif
extern "C" int etg_rollout_wave_cycles(EtgHandle* h, int64_t* cycles, int capacity, int* launches, int* waves, void* stream) {
  CHECK_HANDLE(h);
  if (!launches || !waves) return fail(ETG_ERR_BAD_ARG, "etg_rollout_wave_cycles: launches / waves are null");
  *launches = h->wc_launches;
  *waves = h->wc_waves;
  if (!cycles) return ETG_OK;      // the size query
  if (capacity < h->wc_launches * h->wc_waves) return fail(ETG_ERR_BAD_ARG, "etg_rollout_wave_cycles: the buffer is too small");
  if (h->wc_launches > 0)
    HIP_TRY(hipMemcpyAsync(cycles, h->wave_cycles, (size_t)h->wc_launches * h->wc_waves * sizeof(long long), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return ETG_OK;
}

extern "C" int etg_set_rollout_mode(EtgHandle* h, int simulate_finished) {
  CHECK_HANDLE(h);
  h->K.stop_at_done = simulate_finished ? 0 : 1;
  return ETG_OK;
}

extern "C" int etg_episode_stats(EtgHandle* h, float* ret, int32_t* len, void* stream) {
  CHECK_HANDLE(h);
  hipLaunchKernelGGL(k_episode_stats, dim3((h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, ret, len);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// A rollout of n_steps control steps as fused launches of at most h->rollout_chunk steps: body(first_step, m) enqueues the launch
// of the steps [first_step, first_step + m) and what follows it, once the sensor-noise stream has moved on by the m observations
// per robot the launch writes.  A non-zero return of the body ends the rollout with that code.
template <class Body> static inline int for_each_chunk(EtgHandle* h, int n_steps, Body&& body) {
  for (int first_step = 0; first_step < n_steps; first_step += h->rollout_chunk) {
    const int m = n_steps - first_step < h->rollout_chunk ? n_steps - first_step : h->rollout_chunk;
    advance_obs_stream(h, m);
    if (int rc = body(first_step, m)) return rc;
  }
  return ETG_OK;
}
// the end of a rollout call: launch errors, then the episode statistics if the caller asked for them
static int rollout_end(EtgHandle* h, float* ret, int32_t* len, void* stream) {
  HIP_TRY(hipGetLastError());
  if (ret || len) return etg_episode_stats(h, ret, len, stream);
  return ETG_OK;
}

// n_steps x env.step(action = 0) enqueued back-to-back on the stream (pretrain.py:129-154).
// The same source as etg_step in another kernel: the compiler contracts multiply-adds differently in the two contexts, so the
// two agree to rounding noise amplified by the contacts (joints ~1e-6 rad after one control step), not bit for bit.  The
// per-robot return/length since the last etg_reset are accumulated inside the kernels with alive masking.
extern "C" int etg_rollout_openloop(EtgHandle* h, int n_steps, float* obs, float* ret, int32_t* len, void* stream) {
  CHECK_HANDLE(h);
  if (n_steps <= 0 || !ret || !len) return fail(ETG_ERR_BAD_ARG, "etg_rollout_openloop: bad arguments");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_rollout_openloop: call etg_reset first");
  if (h->K.motor_mode != 2) {
    // fused: up to rollout_chunk control steps per launch, everything in registers in between
    const dim3 grid = tick_grid(h);
    hipStream_t s = (hipStream_t)stream;
    // per-wave cycle counters of this call's launches (etg_rollout_wave_cycles): one 8-byte store per wave and launch
    const int n_launch = (n_steps + h->rollout_chunk - 1) / h->rollout_chunk, n_waves = (int)grid.x;
    if (h->wc_cap < n_launch * n_waves) {
      if (h->wave_cycles) (void)hipFree(h->wave_cycles);
      h->wave_cycles = nullptr;
      h->wc_cap = 0;
      if (hipMalloc((void**)&h->wave_cycles, (size_t)n_launch * n_waves * sizeof(long long)) == hipSuccess) h->wc_cap = n_launch * n_waves;
    }
    h->wc_launches = h->wave_cycles ? n_launch : 0;
    h->wc_waves = n_waves;
    for_each_chunk(h, n_steps, [&](int first_step, int m) {
      const int launch = first_step / h->rollout_chunk;
      const bool last = first_step + m == n_steps;
      // stop_at_done: a robot's last row is written by the launch its episode ends in -- every launch writes to the caller's rows
      float* o = (obs && (last || h->K.stop_at_done)) ? obs : h->tmp_obs;
      long long* cyc = h->wave_cycles ? h->wave_cycles + (size_t)launch * n_waves : nullptr;
      const StatOut so = last ? StatOut{ret, (int*)len, cyc} : StatOut{nullptr, nullptr, cyc};
      LAUNCH_TICK(k_rollout16, k_rollout, grid, s, h->K, h->D, m, o, so);
      if (o == obs) launch_rollout_noise(h, m, obs, s);
      return ETG_OK;
    });
    HIP_TRY(hipGetLastError());
    return ETG_OK;
  } else {
    for (int k = 0; k < n_steps; k++) {
      float* o = (obs && k == n_steps - 1) ? obs : h->tmp_obs;
      int rc = etg_step(h, nullptr, nullptr, o, h->tmp_reward, h->tmp_done, nullptr, stream);
      if (rc != ETG_OK) return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  return etg_episode_stats(h, ret, len, stream);
}

extern "C" int etg_rollout_actions(EtgHandle* h, const float* actions, int n_steps, float* obs, float* rec_joint_angle, float* rec_imu,
                                   float* rec_obs, float* rec_reward, uint8_t* rec_done, float* ret, int32_t* len, void* stream) {
  CHECK_HANDLE(h);
  if (!actions || n_steps <= 0 || !obs) return fail(ETG_ERR_BAD_ARG, "etg_rollout_actions: actions / obs null or n_steps <= 0");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_rollout_actions: call etg_reset first");
  if (h->K.motor_mode == 2) return fail(ETG_ERR_STATE, "etg_rollout_actions: POSITION / TORQUE commands only ([n_steps,N,12] tapes)");
  if (h->K.noise_on && rec_obs) return fail(ETG_ERR_STATE, "etg_rollout_actions: per-step observations are recorded without sensor noise; switch it off");
  hipStream_t s = (hipStream_t)stream;
  const size_t N = h->N;
  const int rc = for_each_chunk(h, n_steps, [&](int d0, int m) -> int {
    const TapeOut T = {rec_joint_angle ? rec_joint_angle + (size_t)d0 * N * ETG_ACT_DIM : nullptr, rec_imu ? rec_imu + (size_t)d0 * N * 6 : nullptr,
                       rec_obs ? rec_obs + (size_t)d0 * N * ETG_OBS_DIM : nullptr, rec_reward ? rec_reward + (size_t)d0 * N : nullptr,
                       rec_done ? rec_done + (size_t)d0 * N : nullptr};
    const float* a = actions + (size_t)d0 * N * ETG_ACT_DIM;
    LAUNCH_TICK(k_rollout_actions16, k_rollout_actions, tick_grid(h), s, h->K, h->D, m, a, obs, T);
    launch_rollout_noise(h, m, obs, s);
    // the last step of EVERY launch writes its row to `obs`, not to the tape: the tape gets its copy per chunk (rows 49, 99,
    // ... and n_steps - 1; recorded observations carry no sensor noise, which the check above enforces)
    if (rec_obs)
      HIP_TRY(hipMemcpyAsync(rec_obs + (size_t)(d0 + m - 1) * N * ETG_OBS_DIM, obs, N * ETG_OBS_DIM * sizeof(float), hipMemcpyDeviceToDevice, s));
    return ETG_OK;
  });
  if (rc) return rc;
  return rollout_end(h, ret, len, stream);
}

// ---- the closed-loop entry points (etg_rollout_policy, etg_rollout_policy_record, etg_step_policy): what they ask of the
// policy, and the two forms its weights are handed to the kernels in.  fn: the entry point's name for the error text
// n_scan: the actor's last n_scan columns are scan columns the kernel computes itself (include/etgsim_scan_policy.h)
static int policy_checks(const char* fn, const EtgHandle* h, const EtgPolicy* pol, int obs_col0, int n_scan = 0) {
  // (a wider policy -- etg_policy_create takes up to 512 columns -- has neither the 4 k-blocks of w1 nor the per-wave stream)
  if (pol->in_dim > 4 * pol::KQ1)
    return fail(ETG_ERR_BAD_ARG, std::string(fn) + ": the fused closed-loop kernels take a policy of in_dim <= 64 (wider ones: "
                                                   "etg_policy_forward / etg_policy_sample, then etg_step)");
  if (pol->device != h->device) return fail(ETG_ERR_BAD_ARG, std::string(fn) + ": policy and simulator live on different devices");
  if (obs_col0 < 0 || obs_col0 + pol->in_dim - n_scan > ETG_OBS_DIM || pol->out_dim != ETG_ACT_DIM)
    return fail(ETG_ERR_BAD_ARG, std::string(fn) + ": the policy must map observation columns [col0, col0 + in_dim) to 12 actions");
  return ETG_OK;
}
// the 16-robot tile's fragments (the bf16 kernels read the bf16 copies packed at load time)
static PolicyW policy_tile(const EtgPolicy* pol, bool bf, int obs_col0) {
  return {(const float4*)(bf ? pol->w1h : pol->w1), (const float4*)(bf ? pol->w2h : pol->w2), (const float4*)(bf ? pol->w3h : pol->w3),
          pol->b1, pol->b2, pol->b3, pol->in_dim, pol->out_dim, obs_col0};
}
// the per-wave kernels' streams (PolicyW: w1 = both hidden layers, w2 unused)
static PolicyW policy_wave(const EtgPolicy* pol, int obs_col0) {
  return {(const float4*)pol->w12q, nullptr, (const float4*)pol->w3q, pol->b1, pol->b2, pol->b3, pol->in_dim, pol->out_dim, obs_col0};
}

// The closed-loop rollout on the 16-lane mapping, for etg_rollout_policy (rec == nullptr) and etg_rollout_policy_record (rec: the
// [n_steps][N][...] arrays of the whole rollout; the _rec kernels get each chunk's part of them and the log-std head).
// precision 0: one wave per workgroup, the policy tile per wave (k_rollout_policy16w: no workgroup barrier); precision 1 (bf16
// operands, an opt-in arithmetic): the 16-robot tile of 4 waves (k_rollout_policy16)
static int rollout_policy16(EtgHandle* h, EtgPolicy* pol, int n_steps, float act_scale, int precision, int obs_col0, float* obs,
                            const RecOut* rec, float* ret, int32_t* len, void* stream) {
  const bool bf = precision != 0;
  const bool per_wave = precision == 0;   // (policy_checks has refused every policy the per-wave tile does not take)
  const PolicyW P = per_wave ? policy_wave(pol, obs_col0) : policy_tile(pol, bf, obs_col0);
  const dim3 g = per_wave ? dim3(h->N / 4) : dim3(h->N / 16), b = per_wave ? dim3(BLOCK) : dim3(256);
  hipStream_t s = (hipStream_t)stream;
  const size_t N = h->N;
  for_each_chunk(h, n_steps, [&](int d0, int m) {
    RecOut R = {};
    if (rec)
      R = {rec->obs + (size_t)d0 * N * ETG_OBS_DIM, rec->act + (size_t)d0 * N * ETG_ACT_DIM, rec->rew + (size_t)d0 * N, rec->done + (size_t)d0 * N,
           rec->noise ? rec->noise + (size_t)d0 * N * ETG_ACT_DIM : nullptr,
           (const float4*)(per_wave ? pol->w3sq : pol->w3sh), pol->b3s};
    dispatch16(h->K, [&](auto f_, auto k_, auto p_) {
      constexpr bool F = ETG_V(f_), KN = ETG_V(k_), PL = ETG_V(p_);
      if (rec) {
        if (per_wave) hipLaunchKernelGGL((k_rollout_policy16w_rec<F, KN, PL>), g, b, 0, s, h->K, h->D, P, m, act_scale, obs, R);
        else hipLaunchKernelGGL((k_rollout_policy16_rec<F, KN, PL>), g, b, 0, s, h->K, h->D, P, m, act_scale, obs, R);
      } else {
        if (per_wave) hipLaunchKernelGGL((k_rollout_policy16w<F, KN, PL>), g, b, 0, s, h->K, h->D, P, m, act_scale, obs);
        else hipLaunchKernelGGL((k_rollout_policy16<F, KN, PL>), g, b, 0, s, h->K, h->D, P, m, act_scale, obs);
      }
    });
    launch_rollout_noise(h, m, obs, s);   // every chunk ends in the caller's rows: the next chunk reads them
    return ETG_OK;
  });
  return rollout_end(h, ret, len, stream);
}

extern "C" int etg_rollout_policy(EtgHandle* h, EtgPolicy* pol, int n_steps, float act_scale, int precision, int obs_col0,
                                  float* obs, float* ret, int32_t* len, void* stream) {
  CHECK_HANDLE(h);
  if (!pol || n_steps <= 0 || !obs) return fail(ETG_ERR_BAD_ARG, "etg_rollout_policy: bad arguments");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_rollout_policy: call etg_reset first");
  if (int rc = policy_checks("etg_rollout_policy", h, pol, obs_col0)) return rc;
  if (h->K.motor_mode == 2 || (h->lanes == 16 ? h->N % 16 != 0 : h->N % 64 != 0))
    return fail(ETG_ERR_STATE, "etg_rollout_policy: needs POSITION/TORQUE mode and whole workgroups: num_envs % 16 == 0 on the 16-lane "
                               "mapping (16 robots per workgroup), num_envs % 64 == 0 on the 4-lane one (64 per workgroup)");
  if (h->lanes == 16) return rollout_policy16(h, pol, n_steps, act_scale, precision, obs_col0, obs, nullptr, ret, len, stream);
  // the 4-lane mapping: 64 robots per workgroup, two stacked policy tiles per pass (k_rollout_policy4)
  const bool bf = precision != 0;
  const PolicyW P = policy_tile(pol, bf, obs_col0);
  const dim3 g4(h->N / 64), b(256);
  hipStream_t s = (hipStream_t)stream;
  const int rc = for_each_chunk(h, n_steps, [&](int, int m) {
    int refused = ETG_OK;
    dispatch4(h->K, [&](auto f_, auto p_, auto b_) {
      constexpr bool F = ETG_V(f_), PL = ETG_V(p_);
      constexpr int BODY = ETG_V(b_);
      if constexpr (BODY == 3)   // (the closed-loop kernel is not instantiated with three body rows per leg: callers step instead)
        refused = fail(ETG_ERR_STATE, "etg_rollout_policy: body_contacts = 3 is served by etg_step / etg_rollout_openloop / etg_rollout_actions");
      else if (!bf) hipLaunchKernelGGL((k_rollout_policy4<F, false, PL, BODY>), g4, b, 0, s, h->K, h->D, P, m, act_scale, obs);
      else hipLaunchKernelGGL((k_rollout_policy4<F, true, PL, BODY>), g4, b, 0, s, h->K, h->D, P, m, act_scale, obs);
    });
    if (!refused) launch_rollout_noise(h, m, obs, s);
    return refused;
  });
  if (rc) return rc;
  return rollout_end(h, ret, len, stream);
}

extern "C" int etg_rollout_policy_record(EtgHandle* h, EtgPolicy* pol, int n_steps, float act_scale, int precision, int obs_col0,
                                         float* obs, const float* noise, float* rec_obs, float* rec_act, float* rec_reward,
                                         uint8_t* rec_done, float* ret, int32_t* len, void* stream) {
  CHECK_HANDLE(h);
  if (!pol || n_steps <= 0 || !obs || !rec_obs || !rec_act || !rec_reward || !rec_done)
    return fail(ETG_ERR_BAD_ARG, "etg_rollout_policy_record: bad arguments");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_rollout_policy_record: call etg_reset first");
  if (noise && !pol->has_std) return fail(ETG_ERR_STATE, "etg_rollout_policy_record: a stochastic rollout needs etg_policy_load_std() first");
  if (int rc = policy_checks("etg_rollout_policy_record", h, pol, obs_col0)) return rc;
  if (h->lanes != 16 || h->N % 16 != 0 || h->K.motor_mode == 2)
    return fail(ETG_ERR_STATE, "etg_rollout_policy_record: needs the 16-lanes-per-robot mapping, num_envs % 16 == 0, POSITION/TORQUE mode");
  const RecOut rec = {rec_obs, rec_act, rec_reward, rec_done, noise, nullptr, nullptr};
  return rollout_policy16(h, pol, n_steps, act_scale, precision, obs_col0, obs, &rec, ret, len, stream);
}

// The refusals that etg_step_policy and the collect entry points share, in this order (k_step_policy16 / k_collect_policy16 run
// the fp32 per-wave actor tile only; policy_checks has already refused a policy wider than its 64 columns)
static int step_policy_checks(const char* fn_, const EtgHandle* h, const EtgPolicy* pol, int precision, int obs_col0, const float* noise,
                              int n_scan = 0) {
  const std::string fn(fn_);
  if (noise && !pol->has_std) return fail(ETG_ERR_STATE, fn + ": sampling needs etg_policy_load_std() first");
  if (int rc = policy_checks(fn_, h, pol, obs_col0, n_scan)) return rc;
  if (precision != 0) return fail(ETG_ERR_BAD_ARG, fn + ": the kernel runs the fp32 per-wave actor tile: precision 0, in_dim <= 64");
  if (h->lanes != 16 || h->N % 16 != 0)
    return fail(ETG_ERR_BAD_ARG, fn + ": needs the 16-lanes-per-robot mapping and num_envs % 16 == 0");
  if (h->K.motor_mode == 2) return fail(ETG_ERR_BAD_ARG, fn + ": the HYBRID motor mode is not covered (its action has 60 columns)");
  if (h->K.noise_on) return fail(ETG_ERR_BAD_ARG, fn + ": sensor noise is not covered: switch it off or step");
  return ETG_OK;
}

// One closed-loop control step of every robot (include/etgsim_step_policy.h): k_step_policy16 / k_step_policy16_ar, one launch
// (auto_reset without a cached settle for every robot: the step launch, then etg_reset masked by `done`, as etg_step_autoreset)
extern "C" int etg_step_policy(EtgHandle* h, EtgPolicy* pol, float act_scale, int precision, int obs_col0, int auto_reset,
                               const float* noise, const uint8_t* donef, float* obs, float* act, float* act_obs, float* terminal_obs,
                               float* reward, uint8_t* done, float* info, void* stream) {
  CHECK_HANDLE(h);
  if (!pol || !obs || !terminal_obs || !reward || !done)
    return fail(ETG_ERR_BAD_ARG, "etg_step_policy: policy, obs, terminal_obs, reward and done must be non-null");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_step_policy: call etg_reset first");
  if (int rc = step_policy_checks("etg_step_policy", h, pol, precision, obs_col0, noise)) return rc;
  if (auto_reset) refresh_all_cached(h);
  const bool fused_reset = auto_reset && h->all_cached;
  advance_obs_stream(h, fused_reset ? 2 : 1);
  const PolicyW Pq = policy_wave(pol, obs_col0);
  const StepPolOut O = {noise, (const float4*)pol->w3sq, pol->b3s, donef, act, act_obs, terminal_obs, reward, done, info};
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(h->N / 4);
  if (fused_reset) {
    LAUNCH16(k_step_policy16_ar, g, s, h->K, h->D, Pq, act_scale, obs, O, h->NX);
  } else {
    LAUNCH16(k_step_policy16, g, s, h->K, h->D, Pq, act_scale, obs, O);
  }
  HIP_TRY(hipGetLastError());
  if (auto_reset && !fused_reset) {   // some robot needs a simulated settle: the general reset path masked by the done bytes
    if (h->push_on)
      if (int rc = etg_clear_pushes(h, done, stream)) return rc;
    return etg_reset(h, done, obs, stream);
  }
  return ETG_OK;
}

// The refusals the scan columns add to those of step_policy_checks (include/etgsim_scan_policy.h), before them and before any
// launch.  `wide`: are the wide row arrays all there?
static int scan_policy_checks(const char* fn_, const EtgHandle* h, const EtgPolicy* pol, const float* points, int n_points, float clip,
                              const float* scan, bool wide) {
  const std::string fn(fn_);
  if (!points || !scan || !wide) return fail(ETG_ERR_BAD_ARG, fn + ": points, scan and the wide row arrays must be non-null");
  if (n_points < 1 || n_points > kScanPolMax) return fail(ETG_ERR_BAD_ARG, fn + ": n_points must be in 1..16 (one lane per robot and point)");
  if (pol->in_dim - n_points < 1) return fail(ETG_ERR_BAD_ARG, fn + ": the actor must read at least one observation column before its n_points scan columns");
  if (pol->in_dim > 4 * pol::KQ1) return fail(ETG_ERR_BAD_ARG, fn + ": the actor's observation and scan columns together must be at most 64 (in_dim <= 64)");
  if (clip < 0.0f) return fail(ETG_ERR_BAD_ARG, fn + ": clip must not be negative");
  if (h->K.terrain != 0 && !h->K.hf) return fail(ETG_ERR_STATE, fn + ": call etg_set_heightfield first");
  return ETG_OK;
}

// etg_step_policy with the scan columns computed in the launch (include/etgsim_scan_policy.h): k_step_policy16_scan / _scan_ar
extern "C" int etg_step_policy_scan(EtgHandle* h, EtgPolicy* pol, float act_scale, int precision, int obs_col0, int auto_reset,
                                    const float* noise, const uint8_t* donef, float* obs, float* act, float* act_obs, float* terminal_obs,
                                    float* reward, uint8_t* done, float* info, const float* points, int n_points, float offset, float clip,
                                    float* scan, void* stream) {
  CHECK_HANDLE(h);
  if (!pol || !obs || !reward || !done)
    return fail(ETG_ERR_BAD_ARG, "etg_step_policy_scan: policy, obs, reward and done must be non-null");
  if (int rc = scan_policy_checks("etg_step_policy_scan", h, pol, points, n_points, clip, scan, act_obs && terminal_obs)) return rc;
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_step_policy_scan: call etg_reset first");
  if (int rc = step_policy_checks("etg_step_policy_scan", h, pol, precision, obs_col0, noise, n_points)) return rc;
  if (auto_reset) refresh_all_cached(h);
  const bool fused_reset = auto_reset && h->all_cached;
  advance_obs_stream(h, fused_reset ? 2 : 1);
  const PolicyW Pq = policy_wave(pol, obs_col0);
  const StepPolOut O = {noise, (const float4*)pol->w3sq, pol->b3s, donef, act, act_obs, terminal_obs, reward, done, info};
  const ScanPol Z = {points, n_points, offset, clip, scan};
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(h->N / 4);
  if (fused_reset) {
    LAUNCH16(k_step_policy16_scan_ar, g, s, h->K, h->D, Pq, act_scale, obs, O, h->NX, Z);
  } else {
    LAUNCH16(k_step_policy16_scan, g, s, h->K, h->D, Pq, act_scale, obs, O, Z);
  }
  HIP_TRY(hipGetLastError());
  if (auto_reset && !fused_reset) {   // as etg_step_policy; the reset moved robots, so `scan` is taken again from the live state
    if (h->push_on)
      if (int rc = etg_clear_pushes(h, done, stream)) return rc;
    if (int rc = etg_reset(h, done, obs, stream)) return rc;
    HIP_TRY(etg_height_scan_launch(h->K, h->D.base, nullptr, nullptr, h->N, points, n_points, offset, clip, scan, s));
  }
  return ETG_OK;
}

// n_steps closed-loop control steps with restarts in one launch (include/etgsim_collect.h): k_collect_policy16.  Every refusal
// comes before any launch and before any change to the handle.  etg_collect_policy records no info rows (rec_info = NULL);
// etg_collect_policy_info (include/etgsim_monitor.h) is the same launch with CollectOut::info set.
static int collect_policy_launch(const char* fn_, EtgHandle* h, EtgPolicy* pol, float act_scale, int precision, int obs_col0, int n_steps,
                                 int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                                 float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs, float* rec_terminal,
                                 float* rec_ep_ret, int32_t* rec_ep_len, float* rec_info, void* stream, const ScanPol* Z = nullptr) {
  const std::string fn(fn_);
  CHECK_HANDLE(h);
  if (!pol || !obs || !rec_action || !rec_reward || !rec_done || !rec_terminal || !rec_ep_ret || !rec_ep_len || (!Z && (!rec_obs || !rec_next_obs)))
    return fail(ETG_ERR_BAD_ARG, fn + ": policy, obs and the eight record arrays must be non-null");
  if (Z)   // the scan columns computed in the launch (include/etgsim_scan_policy.h): rec_obs / rec_next_obs are its wide rows
    if (int rc = scan_policy_checks(fn_, h, pol, Z->points, Z->n, Z->clip, Z->scan, rec_obs && rec_next_obs)) return rc;
  if (n_steps < 1) return fail(ETG_ERR_BAD_ARG, fn + ": n_steps must be at least 1");
  if (!h->was_reset) return fail(ETG_ERR_STATE, fn + ": call etg_reset first");
  if (int rc = step_policy_checks(fn_, h, pol, precision, obs_col0, noise, Z ? Z->n : 0)) return rc;
  if (h->NX.ok)
    return fail(ETG_ERR_STATE, fn + ": the handle has prepared next-episode dynamics (etg_prepare_next_dynamics): a second "
                               "restart inside the launch would find no prepared row -- use etg_step_policy");
  refresh_all_cached(h);
  if (!h->all_cached)
    return fail(ETG_ERR_STATE, fn + ": no cached settle for every robot (a full etg_reset, or masked resets that covered "
                               "every robot whose parameters, terrain or start offset changed) -- use etg_step_policy");
  advance_obs_stream(h, 2 * n_steps);   // as n_steps etg_step_policy calls with a fused restart
  const PolicyW Pq = policy_wave(pol, obs_col0);
  const CollectOut R = {noise, (const float4*)pol->w3sq, pol->b3s, donef, rec_obs, rec_action, rec_reward, rec_done,
                        rec_next_obs, rec_terminal, rec_ep_ret, rec_ep_len, rec_info};
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(h->N / 4);
  if (Z) {
    LAUNCH16(k_collect_policy16_scan, g, s, h->K, h->D, Pq, act_scale, obs, R, n_steps, bootstrap_from, *Z);
  } else {
    LAUNCH16(k_collect_policy16, g, s, h->K, h->D, Pq, act_scale, obs, R, n_steps, bootstrap_from);
  }
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_collect_policy(EtgHandle* h, EtgPolicy* pol, float act_scale, int precision, int obs_col0, int n_steps,
                                  int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                                  float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs, float* rec_terminal,
                                  float* rec_ep_ret, int32_t* rec_ep_len, void* stream) {
  return collect_policy_launch("etg_collect_policy", h, pol, act_scale, precision, obs_col0, n_steps, bootstrap_from, noise, donef, obs,
                               rec_obs, rec_action, rec_reward, rec_done, rec_next_obs, rec_terminal, rec_ep_ret, rec_ep_len, nullptr,
                               stream);
}

// the same launch with the step's 64-column info rows recorded too (include/etgsim_monitor.h)
extern "C" int etg_collect_policy_info(EtgHandle* h, EtgPolicy* pol, float act_scale, int precision, int obs_col0, int n_steps,
                                       int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                                       float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs,
                                       float* rec_terminal, float* rec_ep_ret, int32_t* rec_ep_len, float* rec_info, void* stream) {
  if (h && !rec_info) return fail(ETG_ERR_BAD_ARG, "etg_collect_policy_info: rec_info must be non-null");
  return collect_policy_launch("etg_collect_policy_info", h, pol, act_scale, precision, obs_col0, n_steps, bootstrap_from, noise, donef,
                               obs, rec_obs, rec_action, rec_reward, rec_done, rec_next_obs, rec_terminal, rec_ep_ret, rec_ep_len, rec_info,
                               stream);
}

// etg_collect_policy_info (rec_info may be NULL here) with the scan columns computed in the launch (include/etgsim_scan_policy.h)
extern "C" int etg_collect_policy_scan(EtgHandle* h, EtgPolicy* pol, float act_scale, int precision, int obs_col0, int n_steps,
                                       int bootstrap_from, const float* noise, const uint8_t* donef, float* obs, float* rec_obs,
                                       float* rec_action, float* rec_reward, uint8_t* rec_done, float* rec_next_obs,
                                       float* rec_terminal, float* rec_ep_ret, int32_t* rec_ep_len, float* rec_info, const float* points,
                                       int n_points, float offset, float clip, float* scan, void* stream) {
  const ScanPol Z = {points, n_points, offset, clip, scan};
  return collect_policy_launch("etg_collect_policy_scan", h, pol, act_scale, precision, obs_col0, n_steps, bootstrap_from, noise, donef,
                               obs, rec_obs, rec_action, rec_reward, rec_done, rec_next_obs, rec_terminal, rec_ep_ret, rec_ep_len, rec_info,
                               stream, &Z);
}

extern "C" int etg_leg_kinematics(EtgHandle* h, const float* q, int n, float* foot, float* jac, void* stream) {
  CHECK_HANDLE(h);
  if (!q || !foot || n <= 0) return fail(ETG_ERR_BAD_ARG, "etg_leg_kinematics: bad arguments");
  hipLaunchKernelGGL(k_leg_kin, dim3((n + 3) / 4), dim3(BLOCK), 0, (hipStream_t)stream, h->K, h->M, q, n, foot, jac);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// camera images (include/etgsim_render.h): the handle's terrain and geometry packed for the kernel of etg_render.hip
extern "C" int etg_render(EtgHandle* h, const float* state, const int* env_ids, int n, const float* view, const float* proj, int width,
                          int height, uint8_t* rgba, float* depth, int* seg, void* stream) {
  CHECK_HANDLE(h);
  if (!state || !env_ids || !view || !proj || !rgba) return fail(ETG_ERR_BAD_ARG, "etg_render: null argument");
  if (n <= 0) return fail(ETG_ERR_BAD_ARG, "etg_render: n must be positive");
  if (width < 1 || width > 4096 || height < 1 || height > 4096) return fail(ETG_ERR_BAD_ARG, "etg_render: width and height must be in 1..4096");
  if ((uintptr_t)rgba % 4) return fail(ETG_ERR_BAD_ARG, "etg_render: rgba must be 4-byte aligned");
  const long long tiles = (long long)((width + 15) / 16) * ((height + 15) / 16);
  if (tiles * n > (1ll << 24) - 1) return fail(ETG_ERR_BAD_ARG, "etg_render: too many pixels for one call");
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> ids(n);
  HIP_TRY(hipMemcpyAsync(ids.data(), env_ids, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= h->N) return fail(ETG_ERR_BAD_ARG, "etg_render: env id outside [0, N)");
  if (h->K.terrain == 1 && h->hf && !h->hf_range_ok) {
    std::vector<float> hh((size_t)h->K.hf_nx * h->K.hf_ny * h->K.hf_bands);
    HIP_TRY(hipMemcpyAsync(hh.data(), h->hf, hh.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    render::height_range(hh.data(), hh.size(), h->hf_lo, h->hf_hi);
    h->hf_range_ok = true;
  }
  const render::RenderScene S = render::make_render_scene(h->K, h->M, h->hf, h->hf_lo, h->hf_hi);
  HIP_TRY(etg_render_launch(S, state, env_ids, n, view, proj, width, height, rgba, depth, seg, s));
  return ETG_OK;
}

// the terrain height scan (include/etgsim_heightscan.h): argument checks here, the kernels in etg_heightscan.hip
static int scan_args(const char* fn, const EtgHandle* h, bool live, const void* pose, long long M, const float* points, int P, float offset,
                     float clip, const float* out) {
  const std::string f(fn);
  if (!h) return fail(ETG_ERR_BAD_ARG, f + ": null handle");
  if ((!live && !pose) || !points || !out) return fail(ETG_ERR_BAD_ARG, f + ": null argument");
  if (M < 1) return fail(ETG_ERR_BAD_ARG, f + ": M must be at least 1");
  if (P < 1 || P > ETG_HEIGHT_SCAN_MAX_POINTS) return fail(ETG_ERR_BAD_ARG, f + ": P must be in 1..64");
  if (M * P >= (1ll << 31) - 256) return fail(ETG_ERR_BAD_ARG, f + ": M * P must be below 2^31 - 256");
  if (clip < 0.0f) return fail(ETG_ERR_BAD_ARG, f + ": clip must not be negative");
  if (live && !h->was_reset) return fail(ETG_ERR_STATE, f + ": call etg_reset first");
  if (h->K.terrain != 0 && !h->K.hf) return fail(ETG_ERR_STATE, f + ": call etg_set_heightfield first");
  return ETG_OK;
}

extern "C" int etg_scan_pose(EtgHandle* h, float* pose, void* stream) {
  if (!h) return fail(ETG_ERR_BAD_ARG, "etg_scan_pose: null handle");
  if (!pose) return fail(ETG_ERR_BAD_ARG, "etg_scan_pose: null argument");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_scan_pose: call etg_reset first");
  CHECK_HANDLE(h);
  HIP_TRY(etg_scan_pose_launch(h->D.base, h->N, pose, (hipStream_t)stream));
  return ETG_OK;
}

extern "C" int etg_height_scan_at(EtgHandle* h, const float* pose, const int32_t* env_ids, int M, const float* points, int P, float offset,
                                  float clip, float* out, void* stream) {
  if (int rc = scan_args("etg_height_scan_at", h, false, pose, M, points, P, offset, clip, out)) return rc;
  CHECK_HANDLE(h);
  HIP_TRY(etg_height_scan_launch(h->K, h->D.base, pose, env_ids, M, points, P, offset, clip, out, (hipStream_t)stream));
  return ETG_OK;
}

extern "C" int etg_height_scan(EtgHandle* h, const float* points, int P, float offset, float clip, float* out, void* stream) {
  if (int rc = scan_args("etg_height_scan", h, true, nullptr, h ? h->N : 1, points, P, offset, clip, out)) return rc;
  CHECK_HANDLE(h);
  HIP_TRY(etg_height_scan_launch(h->K, h->D.base, nullptr, nullptr, h->N, points, P, offset, clip, out, (hipStream_t)stream));
  return ETG_OK;
}

extern "C" int etg_extra_sensors(EtgHandle* h, const float* obs, float* out, void* stream) {
  CHECK_HANDLE(h);
  if (!obs || !out) return fail(ETG_ERR_BAD_ARG, "etg_extra_sensors: null argument");
  const int total = h->N * ETG_EXTRA_DIM;
  hipLaunchKernelGGL(k_extra_sensors, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->M, h->D, obs, out);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// the extra sensor columns of the terminal rows of the last etg_step_autoreset_terminal (include/etgsim_terminal.h)
extern "C" int etg_extra_sensors_terminal(EtgHandle* h, const float* terminal_obs, const float* terminal_ctx, const uint8_t* done,
                                          float* out, void* stream) {
  CHECK_HANDLE(h);
  if (!terminal_obs || !terminal_ctx || !done || !out) return fail(ETG_ERR_BAD_ARG, "etg_extra_sensors_terminal: null argument");
  if (!h->was_reset) return fail(ETG_ERR_STATE, "etg_extra_sensors_terminal: call etg_reset first");
  const int total = h->N * ETG_EXTRA_DIM;
  hipLaunchKernelGGL(k_extra_sensors_terminal, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->M, h->D,
                     terminal_obs, terminal_ctx, done, out);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_get_state(EtgHandle* h, float* state, void* stream) {
  CHECK_HANDLE(h);
  if (!state) return fail(ETG_ERR_BAD_ARG, "etg_get_state: null");
  hipLaunchKernelGGL(k_get_state, dim3(grid_for(h)), dim3(BLOCK), 0, (hipStream_t)stream, h->K, h->D, state);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// contact impulses of the feet, rows [N,12] <-> the SoA columns leg[LG_LAM + k][4N] (both lane mappings share the layout)
__global__ void __launch_bounds__(256) k_lam_io(KCfg K, DevState D, float* lam, int write) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int NL = 4 * K.n_env;
  if (col >= NL) return;
  const int env = col >> 2, leg = col & 3;
  for (int k = 0; k < 4; k++) {   // LG_LAM .. LG_LAMB: the foot's (n, t1, t2) and the body contact's normal
    float* cell = D.leg + (size_t)(LG_LAM + k) * NL + col;
    if (write) *cell = lam[(size_t)env * 16 + 4 * leg + k];
    else lam[(size_t)env * 16 + 4 * leg + k] = *cell;
  }
}
extern "C" int etg_get_contact_impulses(EtgHandle* h, float* lam, void* stream) {
  CHECK_HANDLE(h);
  if (!lam) return fail(ETG_ERR_BAD_ARG, "etg_get_contact_impulses: null");
  hipLaunchKernelGGL(k_lam_io, dim3((4 * h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, lam, 0);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}
extern "C" int etg_set_contact_impulses(EtgHandle* h, const float* lam, void* stream) {
  CHECK_HANDLE(h);
  if (!lam) return fail(ETG_ERR_BAD_ARG, "etg_set_contact_impulses: null");
  hipLaunchKernelGGL(k_lam_io, dim3((4 * h->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->K, h->D, const_cast<float*>(lam), 1);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

extern "C" int etg_set_state(EtgHandle* h, const float* state, void* stream) {
  CHECK_HANDLE(h);
  if (!state) return fail(ETG_ERR_BAD_ARG, "etg_set_state: null");
  hipLaunchKernelGGL(k_set_state, dim3(grid_for(h)), dim3(BLOCK), 0, (hipStream_t)stream, h->K, h->D, state);
  HIP_TRY(hipGetLastError());
  return ETG_OK;
}

// ---- snapshots (include/etgsim_snapshot.h): the RECORD rows of kHandleArrays, in the table's order, as the segments of a
// record; the kernel is etg_snapshot.hip's.
static snapshot::Table snapshot_table(EtgHandle* h) {
  snapshot::Table T;
  int off = snapshot::kHeadWords, n = 0;
  for (const HandleArray& a : kHandleArrays) {
    if (a.use != RECORD) continue;
    T.seg[n++] = snapshot::Seg{*array_slot(h, a), off, a.rows, a.per, a.bytes};
    off += a.rows * a.per;
  }
  T.nseg = n;
  T.row_words = (off + 3) / 4 * 4;
  T.n_env = h->N;
  return T;
}
static uint64_t snapshot_mix(uint64_t a, uint64_t v) { return (a ^ v) * 0x100000001B3ull; }   // FNV-1a over 64-bit words
static uint64_t snapshot_mix(uint64_t a, float v) { uint32_t u; memcpy(&u, &v, 4); return snapshot_mix(a, (uint64_t)u); }
// the layout constants: every segment's place and shape, and the row constants whose order inside a segment could move
static uint64_t snapshot_layout_fp(const snapshot::Table& T) {
  uint64_t a = 0xCBF29CE484222325ull;
  for (int s = 0; s < T.nseg; s++)
    for (int v : {T.seg[s].off, T.seg[s].rows, T.seg[s].per, T.seg[s].bytes}) a = snapshot_mix(a, (uint64_t)v);
  for (int v : {T.row_words, (int)RING, (int)CT_RET, (int)CT_FEXT, (int)CT_PUSH, (int)IC_TICK, (int)IC_OBS_CALL, (int)LC_LAST_FOOT_X,
                (int)PR_DERIVED, (int)PR_STR, (int)FIN_OBS, (int)FIN_OK, (int)ETG_OBS_DIM, (int)ETG_DYN_DIM})
    a = snapshot_mix(a, (uint64_t)v);
  return a;
}
// the configuration that gives a record its meaning (the lane mapping is not part of it: both share the layout)
static uint64_t snapshot_config_fp(const KCfg& K) {
  uint64_t a = 0xCBF29CE484222325ull;
  for (int v : {K.action_repeat, K.settle_ticks, K.motor_mode, K.enable_filter, K.enable_interp, K.pd_n, K.knee, K.etg_on, K.terrain,
                K.terrain ? K.hf_nx : 0, K.terrain ? K.hf_ny : 0, K.terrain ? K.hf_bands : 0})
    a = snapshot_mix(a, (uint64_t)(uint32_t)v);
  for (float v : {K.dt, K.etg_dt, K.pd_a, K.fb[0], K.fb[1], K.fb[2], K.fa[0], K.fa[1], K.fa[2], K.terrain ? K.hf_cell : 0.0f,
                  K.terrain ? K.hf_x0 : 0.0f, K.terrain ? K.hf_y0 : 0.0f})
    a = snapshot_mix(a, v);
  return a;
}
// the ids of a call on the host (empty for env_ids == NULL), each checked against [0, N)
static int snapshot_ids(const char* fn, EtgHandle* h, const int32_t* env_ids, int n, hipStream_t s, std::vector<int32_t>& ids) {
  ids.clear();
  if (!env_ids) return ETG_OK;
  ids.resize(n);
  HIP_TRY(hipMemcpyAsync(ids.data(), env_ids, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= h->N) return fail(ETG_ERR_BAD_ARG, std::string(fn) + ": env id outside [0, N)");
  return ETG_OK;
}

extern "C" int etg_snapshot_row_bytes(EtgHandle* h) {
  if (!h) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_row_bytes: null handle");
  return snapshot_table(h).row_words * 4;
}

extern "C" int etg_snapshot_save(EtgHandle* h, const int32_t* env_ids, int n, void* rows, EtgSnapshotHeader* hdr, void* stream) {
  if (!h) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_save: null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (!rows || !hdr) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_save: null argument");
  if ((uintptr_t)rows % 16) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_save: rows must be 16-byte aligned");
  if (env_ids ? (n < 1 || n > (1 << 20)) : n != h->N)
    return fail(ETG_ERR_BAD_ARG, "etg_snapshot_save: n must be N without env_ids, 1..1048576 with them");
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> ids;
  if (int rc = snapshot_ids("etg_snapshot_save", h, env_ids, n, s, ids)) return rc;
  refresh_all_cached(h);
  const snapshot::Table T = snapshot_table(h);
  HIP_TRY(etg_snapshot_launch(T, env_ids, n, (uint32_t*)rows, 0, s));
  memset(hdr, 0, sizeof(*hdr));
  hdr->magic = ETG_SNAPSHOT_MAGIC;
  hdr->format = ETG_SNAPSHOT_FORMAT;
  hdr->abi_version = etg_version();
  hdr->row_bytes = T.row_words * 4;
  hdr->layout_fp = snapshot_layout_fp(T);
  hdr->config_fp = snapshot_config_fp(h->K);
  hdr->num_envs = h->N;
  hdr->n = n;
  hdr->whole = env_ids ? 0 : 1;
  hdr->hf_bands = h->K.hf_bands;
  hdr->push_calls = h->push_calls;
  hdr->obs_calls = h->obs_calls;
  hdr->noise_call = h->K.noise_call;
  hdr->was_reset = h->was_reset; hdr->fext_set = h->fext_set; hdr->push_on = h->push_on; hdr->all_cached = h->all_cached;
  hdr->strength_on = h->K.strength_on != 0;
  hdr->next_dyn = h->NX.par != nullptr;
  return ETG_OK;
}

extern "C" int etg_snapshot_restore(EtgHandle* h, const int32_t* env_ids, int n, const void* rows, const EtgSnapshotHeader* hdr, void* stream) {
  if (!h) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (!rows || !hdr) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: null argument");
  if ((uintptr_t)rows % 16) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: rows must be 16-byte aligned");
  snapshot::Table T = snapshot_table(h);
  if (hdr->magic != ETG_SNAPSHOT_MAGIC || hdr->format != ETG_SNAPSHOT_FORMAT)
    return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: not a snapshot header of this format");
  if (hdr->abi_version != etg_version()) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: the snapshot is of another library version");
  if (hdr->row_bytes != T.row_words * 4 || hdr->layout_fp != snapshot_layout_fp(T))
    return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: the snapshot's record layout differs from this library's");
  if (hdr->config_fp != snapshot_config_fp(h->K) || hdr->hf_bands != h->K.hf_bands)
    return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: the snapshot was saved under another configuration (time step, action repeat, "
                                 "settle ticks, motor mode, filter / interpolation, pd_latency, body_contacts or terrain)");
  if (hdr->n < 1 || (env_ids ? (n < 1 || n > hdr->n) : (n != h->N || !hdr->whole || hdr->num_envs != h->N || hdr->n != h->N)))
    return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: n must be 1..(records saved) with env_ids; without them the snapshot must be a "
                                 "whole one of exactly this handle's N robots");
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> ids;
  if (int rc = snapshot_ids("etg_snapshot_restore", h, env_ids, n, s, ids)) return rc;
  if (env_ids) {
    std::vector<unsigned char> seen(h->N, 0);
    for (int i = 0; i < n; i++) {
      if (seen[ids[i]]) return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: duplicate target env id");
      seen[ids[i]] = 1;
    }
    if (h->K.terrain == 1 && h->K.hf_bands > 1) {   // a record's settle cache and history belong to the band it was saved on
      std::vector<int32_t> src(n);
      HIP_TRY(hipMemcpy2DAsync(src.data(), sizeof(int32_t), rows, (size_t)hdr->row_bytes, sizeof(int32_t), (size_t)n, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (int i = 0; i < n; i++)
        if (src[i] < 0 || src[i] % h->K.hf_bands != ids[i] % h->K.hf_bands)
          return fail(ETG_ERR_BAD_ARG, "etg_snapshot_restore: a target env id is on another heightfield band than the robot its record was saved from");
    }
  }
  if (hdr->next_dyn && !h->nx_mask) {   // the records carry rows for the next episodes: the arrays of etg_prepare_next_dynamics
    if (int rc = ensure_next_arrays(h, "etg_snapshot_restore", s)) return rc;
    T = snapshot_table(h);
  }
  HIP_TRY(etg_snapshot_launch(T, env_ids, n, (uint32_t*)const_cast<void*>(rows), 1, s));
  refresh_all_cached(h);
  h->inval_seq++;   // a count of uncached robots reported by an earlier masked reset no longer describes the arrays
  if (!env_ids) {
    h->push_calls = hdr->push_calls;
    h->obs_calls = hdr->obs_calls;
    h->K.noise_call = hdr->noise_call;
    h->was_reset = hdr->was_reset != 0;
    h->fext_set = hdr->fext_set != 0;
    h->push_on = hdr->push_on != 0;
    h->all_cached = hdr->all_cached != 0;
    h->K.strength_on = hdr->strength_on;
  } else {   // some robots: the others keep theirs, so a flag holds if either side needs it (all_cached: if both sides have it)
    h->was_reset = h->was_reset || hdr->was_reset;
    h->fext_set = h->fext_set || hdr->fext_set;
    h->push_on = h->push_on || hdr->push_on;
    h->all_cached = h->all_cached && hdr->all_cached;
    h->K.strength_on = h->K.strength_on || hdr->strength_on;
  }
  h->K.ext_force = h->fext_set || h->push_on;
  return ETG_OK;
}
#endif   // ETG_TU_HOST
