"""The variant x entry-point matrix of the physics tick (test infrastructure; imports the oracle, makes no GPU call at import).

etg_kernels.hip instantiates every tick-kernel template once per compile-time variant (ETG_VARIANTS16 / ETG_VARIANTS4 of
etg_layout.h), and every instantiation is a code object of its own: its own register allocation, spills and `if constexpr`
paths.  This module names, for every variant, a configuration that dispatches to it (CONFIGS), for every C-ABI call that
launches a tick kernel the template it launches (ENTRY_POINTS).  A cell
of the matrix is (config, entry point): ONE control step from a synchronised state, judged by tests/parity_util.one_step_verdict
against an OracleEnsemble built from the configuration's own EtgConfig -- the recipe of tests/test_gpu_parity5.py:

  * a `run` device makes a trajectory with step() under U(-AMP, AMP) residual actions and per-robot gaits; before the run
    steps CHECKPOINTS its state, contact impulses and observation rows are taken;
  * at each checkpoint they are installed in the probe (set_state, set_contact_impulses, obs rows) and in the ensemble
    (set_state, set_lambda); the probe takes exactly one control step through its entry point, the ensemble step(action)
    with the action the entry point reports.  The state carries no step counter, and the gait phase is a function of it: a
    step from the run's state under another phase is a 0.2 .. 0.5 rad jump of the joint targets, not the trajectory's
    step.  So the checkpoints are consecutive, and probe and ensemble first take WARMUP plain step() calls with a zero
    action from their reset: their counters then stay with the run's, one entry-point launch per checkpoint and no other;
  * in the variants with body rows every other robot starts the trajectory from a nose-up trunk (pitched_start): its rear
    knees and shins are inside the margin and carry load again when the trunk comes down (run steps 4 .. 6), where the
    walking robots' own knees touch too;
  * the verdict (judge / green): joints (state columns 13:25) within FLOOR_Q, pose (0:7) within FLOOR_P -- the floors of
    tests/test_gpu_parity5.py --, no (robot, checkpoint) pair off every branch, every state finite, and at least as many
    pairs on the nominal branch as the worst ensemble member has when it is judged leave-one-out against the others by
    the same function, less one pair per 64 (the allowance parity_util.sens_tally grants for a lone parting).

tests/test_variant_matrix_cases.py runs the reference-only conditions, the dispatch checks and the `step` column through the
host build of the kernel source; tests/test_gpu_variant_matrix.py runs every cell on the device."""
import functools
import os
import re

import numpy as np

from paddlerobotics_amd import a1_model as A
from tests.parity_controls import gaits, rolling_hills
from tests.parity_util import NCPU, OracleEnsemble, one_step_verdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddlerobotics_amd", "csrc")

FLOOR_Q, FLOOR_P = 2e-5, 1e-5            # rad; m / quaternion: the floors of tests/test_gpu_parity5.py
QCOLS, PCOLS = slice(13, 25), slice(0, 7)
N_OF = {16: 32, 4: 64}                   # 8 waves of 4 robots; 4 waves of 16 (one workgroup of the 4-lane closed-loop kernel)
SETTLE_TICKS = 100
AMP = 0.15                               # residual actions of the trajectory
CHECKPOINTS = (4, 5, 6)                  # run steps whose start state is probed: consecutive, after WARMUP steps
WARMUP = CHECKPOINTS[0]                  # step() calls that bring a probe's step counter (the gait phase) to the run's
SCALE = 0.3                              # act_scale of the closed-loop entry points
N_FORCED = 4                             # robots whose episode the auto-reset entry points end at the last checkpoint
RESET_ROW_BOUND = 1e-6                   # restarted rows against the reset observation (tests/test_gpu_step_policy.py)
TORQUE_LIMIT = 20.0                      # N m: motor_torque_limits of the all-options configurations
DYN_FOOT_FRICTION = 1                    # dynamic-row column (a1_model.dynamic_dict_to_row)


# ---- the configurations: one per variant tuple ---------------------------------------------------------------------------

class Config:
    """lanes, the tuple dispatch16 / dispatch4 must pick -- (FLAT, KNEE, PLAIN) on 16 lanes, (FLAT, PLAIN, BODY) on 4 --, the
    terrain, body_contacts and whether the robot layer's options are on.  Every variant with PLAIN = 0 runs the stateless
    options: a constant lateral force of about 10 N, motor strength ratios U(0.7, 1), motor_torque_limits and
    enable_clip_motor_commands.  (Action filter, action interpolation, pd_latency, sensor noise, random pushes and the
    HYBRID mode carry per-robot history that set_state does not install, or the fused kernels refuse them.)"""

    def __init__(self, lanes, variant, flat, body_contacts, options):
        self.lanes, self.variant, self.flat, self.body_contacts, self.options = lanes, tuple(variant), flat, body_contacts, options
        self.n = N_OF[lanes]
        self.body_rows = body_contacts != 0
        self.name = "%d-%s" % (lanes, "".join(str(v) for v in self.variant))
        self.seed = 100 * lanes + sum(v << (2 * i) for i, v in enumerate(self.variant))

    def heightfield(self):
        return None if self.flat else rolling_hills()

    def env_kw(self):
        """make_env keywords (num_envs, device and auto_reset are the cell's)"""
        kw = dict(lanes_per_robot=self.lanes, settle_ticks=SETTLE_TICKS, body_contacts=self.body_contacts)
        if not self.flat:
            kw.update(task="heightfield", heightfield=self.heightfield())
        if self.options:
            kw.update(motor_torque_limits=TORQUE_LIMIT, enable_clip_motor_commands=True)
        return kw

    def cfg(self):
        """the EtgConfig make_env builds from env_kw() (env.py: BatchedQuadrupedEnv.__init__), for the CPU side"""
        hf = self.heightfield()
        return A.default_config(self.n, settle_ticks=SETTLE_TICKS, terrain=0 if self.flat else 1, heightfield=hf,
                                lanes_per_robot=self.lanes, body_contacts=self.body_contacts,
                                clip_motor_commands=0.2 if self.options else 0.0, torque_limit=TORQUE_LIMIT if self.options else 0.0)

    def force(self):
        """[n,3] N: 8 .. 12 N to the left or to the right, or None"""
        if not self.options:
            return None
        f = np.zeros((self.n, 3), dtype=np.float32)
        f[:, 1] = np.linspace(8.0, 12.0, self.n) * np.where(np.arange(self.n) % 4 < 2, 1.0, -1.0)
        return f

    def strength(self):
        """[n,12] motor strength ratios U(0.7, 1), or None"""
        if not self.options:
            return None
        return np.random.default_rng(self.seed + 7).uniform(0.7, 1.0, size=(self.n, 12)).astype(np.float32)

    def gaits(self):
        return _gaits(self.n, self.seed)

    def actions(self):
        """[steps, n, 12] fp32: the trajectory's residual actions"""
        return np.random.default_rng(self.seed + 100).uniform(-AMP, AMP, size=(CHECKPOINTS[-1] + 1, self.n, 12)).astype(np.float32)

    def forced(self):
        """the robots whose episode the auto-reset entry points end at the last checkpoint: both kinds of start, three waves"""
        m = np.zeros(self.n, dtype=bool)
        m[[1, 6, self.n // 2, self.n - 1][:N_FORCED]] = True
        return m


@functools.lru_cache(maxsize=None)
def _gaits(n, seed):
    return gaits(n, seed)


CONFIGS = [
    # 16 lanes per robot: (FLAT, KNEE, PLAIN)
    Config(16, (1, 1, 1), True, 2, False),
    Config(16, (1, 0, 1), True, 0, False),
    Config(16, (1, 1, 0), True, 2, True),
    Config(16, (0, 1, 1), False, 2, False),
    Config(16, (0, 0, 1), False, 0, False),
    Config(16, (0, 1, 0), False, 2, True),
    # 4 lanes per robot: (FLAT, PLAIN, BODY)
    Config(4, (1, 0, 3), True, 3, True),
    Config(4, (0, 0, 3), False, 3, True),
    Config(4, (1, 0, 1), True, 2, True),
    Config(4, (0, 0, 1), False, 2, True),
    Config(4, (1, 1, 0), True, 0, False),
    Config(4, (1, 0, 0), True, 0, True),
    Config(4, (0, 1, 0), False, 0, False),
    Config(4, (0, 0, 0), False, 0, True),
]
BY_NAME = {c.name: c for c in CONFIGS}


def pitched_start(st, body_rows):
    """the trajectory's start state from the reset state [n,37]: in the variants with body rows every other robot stands nose
    up by 0.35 .. 0.6 rad, its trunk raised so that the rear feet stay where the ground is (hip 0.18 m behind the centre, foot
    0.228 m under the hip).  The rear knees and shins are then inside the 0.02 m margin; the robot comes down on them and on
    its front feet over the next control steps.  No termination condition is met: the feet stay 0.2 m under the trunk in
    its own frame and the trunk's z axis keeps cos(0.6) = 0.83 > 0.5 of the vertical."""
    st = np.array(st, dtype=np.float64)
    if not body_rows:
        return st
    odd = np.arange(st.shape[0]) % 2 == 1
    th = np.linspace(0.35, 0.6, int(odd.sum()))
    st[odd, 2] += 0.228 * np.cos(th) + 0.16 * np.sin(th) - 0.228
    st[odd, 3:7] = np.stack([np.zeros_like(th), -np.sin(th / 2), np.zeros_like(th), np.cos(th / 2)], axis=1)   # (x, y, z, w)
    return st


def install_host(sim, config, reset=True):
    """the configuration's installers on an OracleSim / OracleEnsemble / EmuSim, in the order the env applies them: terrain,
    motor strength ratios (the settle runs under the motor model), gaits, reset, external force"""
    hf, W, B = config.heightfield(), *config.gaits()
    if hf is not None:
        sim.set_heightfield(hf["heights"])
    if config.options:
        sim.set_motor_strength(config.strength())
    sim.set_params(etg_w=W, etg_b=B)
    if reset:
        sim.reset()
    if config.options:
        sim.set_external_force(config.force())


def make_ensemble(config, cfg=None, foot_friction=0.0):
    """the OracleEnsemble of a configuration (cfg: the env's own EtgConfig; default: config.cfg()).  foot_friction = m: every
    member's foot friction is mis-set by the factor 1 + m (the negative control of tests/parity_controls.py)"""
    cfg = config.cfg() if cfg is None else cfg
    ens = OracleEnsemble(config.n, E=4, seed=config.seed, cfg=type(cfg).from_buffer_copy(cfg), threads=min(16, NCPU))
    if foot_friction:
        dyn = np.tile(A.default_dynamic_row(), (config.n, 1)).astype(np.float32).astype(np.float64)
        dyn[:, DYN_FOOT_FRICTION] *= 1.0 + foot_friction
        ens.set_params(dyn=dyn)
    install_host(ens, config)
    return ens


def ensemble_pass(ens, config, states, lams, actions):
    """the ensemble through the checkpoints: reset and WARMUP zero-action steps (its members' step counters start over and
    advance to the run's, as a fresh probe's), then per checkpoint set_state / set_lambda / step(action) -> per checkpoint dict(nominal [n,37], members [M][n,37], done [n] (any member's),
    loaded [n] ticks with a loaded body row in the nominal member's step)"""
    ens.reset()
    if config.options:
        ens.set_external_force(config.force())
    for _ in range(WARMUP):
        ens.step(np.zeros((config.n, 12), dtype=np.float32), want_info=False)
    out = []
    for st, lam, a in zip(states, lams, actions):
        ens.set_state(np.asarray(st, dtype=np.float64))
        ens.set_lambda(np.asarray(lam, dtype=np.float64))
        ens.nominal.body_stats()
        _, _, done, _ = ens.step(np.asarray(a, dtype=np.float32), want_info=False)
        done = np.asarray(done).astype(bool) | np.any(ens.member_done, axis=0)
        out.append(dict(nominal=ens.get_state(), members=ens.member_states(), done=done,
                        loaded=ens.nominal.body_stats()[:, 1]))
    return out


# ---- the verdict -------------------------------------------------------------------------------------------------------------

def _on_branches(dev, nominal, members, keep):
    nq, aq, _, dq = one_step_verdict(dev[:, QCOLS], nominal[:, QCOLS], [m[:, QCOLS] for m in members], FLOOR_Q)
    npz, ap, _, dp = one_step_verdict(dev[:, PCOLS], nominal[:, PCOLS], [m[:, PCOLS] for m in members], FLOOR_P)
    fin = np.isfinite(dev).all(1)
    return (nq & npz & fin)[keep], (aq & ap & fin)[keep], dq[keep], dp[keep]


def allowance(pairs):
    """one pair per 64: what parity_util.sens_tally grants for a lone parting"""
    return max(1, int(round(pairs / 64.0)))


def judge(dev_states, ens_results, exclude=None):
    """dev_states: per checkpoint the device's state [n,37] after its one step; ens_results: ensemble_pass(); exclude: per
    checkpoint a bool mask of robots left out (restarted by an auto-reset entry point), or None -> the tally: pairs, nominal,
    other, none, member_nominal / member_none (every member's own counts on the nominal branch and on no branch, judged
    leave-one-out against the others),
    worst_member, gap_q / gap_p (largest gap to the nearest member), offenders [(checkpoint, robot, joints gap, pose gap)]"""
    t = dict(pairs=0, nominal=0, other=0, none=0, gap_q=0.0, gap_p=0.0, offenders=[])
    M = len(ens_results[0]["members"])
    member_nominal, member_none = np.zeros(M, dtype=int), np.zeros(M, dtype=int)
    for k, (dev, r) in enumerate(zip(dev_states, ens_results)):
        keep = np.ones(dev.shape[0], dtype=bool) if exclude is None or exclude[k] is None else ~np.asarray(exclude[k], dtype=bool)
        dev = np.asarray(dev, dtype=np.float64)
        on_nom, on_any, dq, dp = _on_branches(dev, r["nominal"], r["members"], keep)
        t["pairs"] += int(keep.sum())
        t["nominal"] += int(on_nom.sum())
        t["other"] += int((on_any & ~on_nom).sum())
        t["none"] += int((~on_any).sum())
        dq, dp = np.where(np.isfinite(dq), dq, np.inf), np.where(np.isfinite(dp), dp, np.inf)
        t["gap_q"], t["gap_p"] = max(t["gap_q"], float(dq.max())), max(t["gap_p"], float(dp.max()))
        for i in np.nonzero(~on_any)[0]:
            t["offenders"].append((k, int(np.nonzero(keep)[0][i]), float(dq[i]), float(dp[i])))
        for m in range(M):
            rest = [x for j, x in enumerate(r["members"]) if j != m]
            m_nom, m_any, _, _ = _on_branches(r["members"][m], r["nominal"], rest, keep)
            member_nominal[m] += int(m_nom.sum())
            member_none[m] += int((~m_any).sum())
    t["member_nominal"], t["member_none"] = member_nominal.tolist(), member_none.tolist()
    t["worst_member"] = int(member_nominal.min())
    t["required"] = t["worst_member"] - allowance(t["pairs"])
    return t


def green(t):
    return t["none"] == 0 and t["nominal"] >= t["required"]


def tally_line(what, t):
    return ("%-44s pairs %3d nominal %3d other %2d none %d | worst member's nominal %3d (required %3d) | gap to the nearest member: "
            "joints %.2e (floor %.0e) pose %.2e (floor %.0e)" % (what, t["pairs"], t["nominal"], t["other"], t["none"], t["worst_member"],
                                                               t["required"], t["gap_q"], FLOOR_Q, t["gap_p"], FLOOR_P))


# ---- a trajectory of the host devices (the fp64 oracle, the host build of the kernel source) --------------------------------------

def host_trajectory(run, config, lam_of):
    """`run` (an installed and reset OracleSim / EmuSim) from pitched_start through config.actions() -> dict(states, lams, obs:
    what the device held before each checkpoint's step; acts: the checkpoints' actions)"""
    run.set_state(pitched_start(run.get_state(), config.body_rows))
    out = dict(states=[], lams=[], acts=[])
    for k, a in enumerate(config.actions()):
        if k in CHECKPOINTS:
            out["states"].append(np.asarray(run.get_state(), dtype=np.float64))
            out["lams"].append(np.asarray(lam_of(run), dtype=np.float64))
            out["acts"].append(a)
        run.step(a)
    return out


# ---- the instantiation table -----------------------------------------------------------------------------------------------------

def _bools(text):
    return tuple(int({"true": 1, "false": 0}.get(x.strip(), x.strip())) for x in text.split(","))


def parse_variants():
    """ETG_VARIANTS16 / ETG_VARIANTS4 of etg_layout.h -> {16: [tuples], 4: [tuples]}"""
    src = open(os.path.join(CSRC, "etg_layout.h")).read().replace("\\\n", " ")
    out = {}
    for lanes in (16, 4):
        body = re.search(r"#define ETG_VARIANTS%d\(X\)(.*)" % lanes, src).group(1)
        out[lanes] = [_bools(m) for m in re.findall(r"X\(([^)]*)\)", body)]
    return out


def parse_instantiations():
    """the ETG_INST* table of etg_kernels.hip -> the set of (kernel template, template arguments as ints): every macro's
    argument lists are read from its own #define, every table line expands through it (ETG_INSTP*: BF from the line)"""
    src = open(os.path.join(CSRC, "etg_kernels.hip")).read().replace("\\\n", " ")
    macros = {}
    for name, body in re.findall(r"#define (ETG_INSTP?(?:16|4))\(KERN,[^)]*\)(.*)", src):
        macros[name] = re.findall(r"KERN<([^>]*)>", body)
    out = set()
    for name, args in re.findall(r"^(ETG_INSTP?(?:16|4))\(([^)]*)\)", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        for tpl in macros[name]:
            if "P" in name[8:]:
                tpl = tpl.replace("BF", args[1])
            out.add((args[0], _bools(tpl)))
    return out


def inst_name(inst):
    return "%s<%s>" % (inst[0], ", ".join(str(v) for v in inst[1]))


# ---- the entry points ---------------------------------------------------------------------------------------------------------------

def _plain(k16, k4):
    return lambda lanes, v: [(k16 if lanes == 16 else k4, v)]


def _with_bf(k16, k4, bf):
    # the 4-lane closed-loop kernel has both precisions: <FLAT, BF16, PLAIN, BODY>; the 16-lane tile is bf16 only: <FLAT, KNEE, PLAIN>
    return lambda lanes, v: [(k16, v) if lanes == 16 else (k4, (v[0], bf) + tuple(v[1:]))]


class EntryPoint:
    """name; lanes it serves; auto_reset: the probe env is made with auto_reset=True; kernels(lanes, variant): the
    instantiation the call launches; serves(config): the predicate (False: the call refuses the configuration);
    run(probe, x): one control step of the probe env (GPU) -> (the action the ensemble gets [n,12] numpy, done [n] numpy bool);
    x: the cell's context (Ctx in tests/test_gpu_variant_matrix.py)"""

    def __init__(self, name, lanes, kernels, run, auto_reset=False, body3=True, actor=None):
        self.name, self.lanes, self.kernels, self.run, self.auto_reset, self.body3, self.actor = name, lanes, kernels, run, auto_reset, body3, actor

    def serves(self, config):
        # (N_OF satisfies the third predicate, num_envs % 16 == 0 on 16 lanes and % 64 == 0 on 4, in every cell)
        return config.lanes in self.lanes and (self.body3 or config.body_contacts != 3)

    def targets(self, config):
        return self.kernels(config.lanes, config.variant) + SETUP_KERNELS(config.lanes, config.variant)


def SETUP_KERNELS(lanes, v):
    """every cell resets its probe env: the settle and the first observation are launches of the same variant (the auto-reset
    cells compare the restarted rows with that observation)"""
    return [("k_settle16", v), ("k_finish16", v)] if lanes == 16 else [("k_settle", v), ("k_finish", v)]


def _np(t):
    return t.detach().cpu().numpy()


def _done_of_len(ln, x):
    # a fused rollout reports no done flags: a robot that is alive after the step of checkpoint k has episode length WARMUP + k + 1
    return _np(ln) != WARMUP + x.k + 1


def _run_step(e, x):
    _, _, done, _ = e.step(x.act, donef=x.donef, want_info=True)
    return _np(x.act), _np(done).astype(bool)


def _run_openloop(e, x):
    _, ln = e.rollout_openloop(1)
    return np.zeros((e.num_envs, 12), dtype=np.float32), _done_of_len(ln, x)


def _run_actions(e, x):
    _, _, rec = e.rollout_actions(x.act.unsqueeze(0), record=("done",))
    return _np(x.act), _np(rec["done"][0]).astype(bool)


def _run_policy(precision):
    def run(e, x):
        _, ln = e.rollout_policy(x.const_policy, 1, SCALE, precision=precision, fused=True)
        return x.const_action, _done_of_len(ln, x)
    return run


def _run_record(precision, noisy):
    def run(e, x):
        _, _, rec = e.rollout_policy_record(x.policy, 1, SCALE, precision=precision, noise=x.noise.unsqueeze(0) if noisy else None)
        return _np(rec["action"][0]) * np.float32(SCALE), _np(rec["done"][0]).astype(bool)
    return run


def _run_step_policy(mode):
    def run(e, x):
        _, _, done, _, act = e.step_policy(x.policy, SCALE, mode, noise=x.noise if mode == "sample" else None, donef=x.donef)
        return _np(act) * np.float32(SCALE), _np(done).astype(bool)
    return run


def _run_collect(want_info):
    def run(e, x):
        out = e.collect_policy(x.policy, 1, SCALE, "sample", noise=x.noise.unsqueeze(0),
                               donef=None if x.donef is None else x.donef.unsqueeze(0), want_info=want_info)
        if want_info:
            assert tuple(out["info"].shape) == (1, e.num_envs, A.INFO_DIM)
        return _np(out["action"][0]) * np.float32(SCALE), _np(out["done"][0]).astype(bool)
    return run


BOTH, L16 = (16, 4), (16,)
ENTRY_POINTS = [
    EntryPoint("step", BOTH, _plain("k_step16", "k_step"), _run_step),
    EntryPoint("step_autoreset", BOTH, _plain("k_step16_ar", "k_step_ar"), _run_step, auto_reset=True),
    EntryPoint("rollout_openloop", BOTH, _plain("k_rollout16", "k_rollout"), _run_openloop),
    EntryPoint("rollout_actions", BOTH, _plain("k_rollout_actions16", "k_rollout_actions"), _run_actions),
    # precision 0 on 16 lanes is the per-wave kernel (rollout_policy16: per_wave), on 4 lanes the fp32 tile; precision 1 on 16
    # lanes is the bf16 16-robot tile, the only k_rollout_policy16 / k_rollout_policy16_rec there is
    EntryPoint("rollout_policy-p0", BOTH, _with_bf("k_rollout_policy16w", "k_rollout_policy4", 0), _run_policy(0), body3=False, actor="const"),
    EntryPoint("rollout_policy-p1", BOTH, _with_bf("k_rollout_policy16", "k_rollout_policy4", 1), _run_policy(1), body3=False, actor="const"),
    EntryPoint("rollout_policy_record-p0", L16, _plain("k_rollout_policy16w_rec", None), _run_record(0, False), actor="mlp"),
    EntryPoint("rollout_policy_record-p0-noise", L16, _plain("k_rollout_policy16w_rec", None), _run_record(0, True), actor="mlp"),
    EntryPoint("rollout_policy_record-p1", L16, _plain("k_rollout_policy16_rec", None), _run_record(1, False), actor="mlp"),
    EntryPoint("rollout_policy_record-p1-noise", L16, _plain("k_rollout_policy16_rec", None), _run_record(1, True), actor="mlp"),
    EntryPoint("step_policy-predict", L16, _plain("k_step_policy16", None), _run_step_policy("predict"), actor="mlp"),
    EntryPoint("step_policy-sample", L16, _plain("k_step_policy16", None), _run_step_policy("sample"), actor="mlp"),
    EntryPoint("step_policy_autoreset-predict", L16, _plain("k_step_policy16_ar", None), _run_step_policy("predict"), auto_reset=True, actor="mlp"),
    EntryPoint("step_policy_autoreset-sample", L16, _plain("k_step_policy16_ar", None), _run_step_policy("sample"), auto_reset=True, actor="mlp"),
    EntryPoint("collect_policy", L16, _plain("k_collect_policy16", None), _run_collect(False), auto_reset=True, actor="mlp"),
    EntryPoint("collect_policy-info", L16, _plain("k_collect_policy16", None), _run_collect(True), auto_reset=True, actor="mlp"),
]
EP_BY_NAME = {e.name: e for e in ENTRY_POINTS}

CELLS = [(c, e) for c in CONFIGS for e in ENTRY_POINTS if e.serves(c)]
REFUSALS = [(c, e) for c in CONFIGS for e in ENTRY_POINTS if not e.serves(c)]


def cell_id(config, ep):
    return "%s-%s" % (config.name, ep.name)


def const_policy_action():
    """the constant actor of the rollout_policy cells: all weights zero, b3 = atanh(a) for 12 distinct a, so that the action is
    tanh(b3) * SCALE in either precision (the biases stay fp32) -> (b3 [12] fp32, the scaled action [12] fp32).  The cell tests
    the physics and the action wiring; the actor arithmetic is tests/test_gpu_policy_narrow.py's."""
    a = np.linspace(-0.5, 0.5, 12)[[7, 2, 10, 0, 5, 11, 3, 8, 1, 9, 4, 6]]
    b3 = np.arctanh(a).astype(np.float32)
    return b3, (np.tanh(b3.astype(np.float64)) * SCALE).astype(np.float32)
