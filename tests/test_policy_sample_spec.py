"""The binary32 specification of the Dreamer agent's sampled modes (tests/policy_sample_spec.c): its scalar
functions against libm, its normal generator's statistics, the independence of a car's draws from the batch, mode `mean` against
PolicySpec, the sampled modes against a float64 restatement of the reference's formulas fed the same normals, and against the NumPy
port's own random stream statistically - from one state and in closed loop on the C oracle; the C-ABI's new symbols."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import policy_sample_spec as pss
from oracle import racecar_oracle as ro
from oracle.dreamer_policy_port import RAW_INIT_STD, DreamerPolicy
from policy_sample_spec import EpisodeClock, PolicySampleSpec
from policy_spec import PolicySpec
from test_golden_policy import GOLDEN, c_env, weights

CHECKPOINTS = sorted(os.path.basename(p)[len("dreamer_policy_"):-4] for p in glob.glob(os.path.join(GOLDEN, "dreamer_policy_*.npz")))
MARGIN = 4.0          # as test_policy_spec.MARGIN: the spec's error against float64 over the float32 restatement's own
# test_sampled_modes_are_the_reference_formulas: by how much the binary32 score DIFFERENCE of two candidates s, t of one car may
# be off, from float64's own quantities.  (1) Rounding inside a score: a term is -n^2 / 2 - 2 (ln 2 - u - softplus(-2 u)), some
# eight roundings (the product, softplus' 3 ulp, two differences, the sums) of intermediates no larger than n^2 / 2 + 2 |u| + 2:
# 8 x 2^-23 = 2^-20 of that sum over both dimensions, for each of the two candidates.  (2) The error the actor's distribution
# inherits from the output layer, documented by item 12 as up to OUT_ERR = 1.2e-3: mu's error shifts all candidates alike and
# enters a difference only through the score's curvature (|f''| <= 2) times u_s - u_t = sd (n_s - n_t); sd's error is at most
# sd OUT_ERR (d softplus = sigmoid <= softplus) and enters through |f'| <= 2 times n_s - n_t: together 4 OUT_ERR sd |n_s - n_t|
# per dimension.
OUT_ERR = 1.2e-3


def _score_gap_bound(mu, sd, cs, ct):
    """mu, sd [n, 2]; cs, ct [n, 2] the normals of the two candidates."""
    rounding = sum((0.5 * c ** 2 + 2 * np.abs(mu + sd * c) + 2).sum(1) for c in (cs, ct)) * 2.0 ** -20
    return rounding + (4 * OUT_ERR * sd * np.abs(cs - ct)).sum(1)


def _ulp_error(got, want64):
    ulp = np.spacing(np.abs(want64.astype(np.float32))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / ulp


def test_log_and_softplus_against_libm():
    """pm_log over every 7th u1 of the Box-Muller grid, both edges (2^-24, 1), a dense grid of [0.5, 2] and 10^6 points of the
    normal range; pm_softplus over the grids of test_policy_spec.  Measured: log 0.82 ulp, softplus 2.76 ulp (at x = -6.2: exp's
    1.03 ulp, the sum 1 + t, log's 0.82 and the quotient's and product's roundings); asserted: 1 and 3.  Beyond |x| = 86 exp
    saturates at exp(-86): softplus returns x, or 4.5e-38 - below anything 0.1 or 1e-4 is added to."""
    x = np.concatenate([np.arange(1, 2 ** 24 + 1, 7, dtype=np.float64) * 2.0 ** -24, [2.0 ** -24, 1.0], np.linspace(0.5, 2.0, 1_000_001),
                        np.geomspace(1e-37, 3e38, 1_000_001)]).astype(np.float32)
    worst_log = float(_ulp_error(pss.scalar_map("log", x), np.log(x.astype(np.float64))).max())
    assert pss.scalar_map("log", np.float32([1.0]))[0] == 0.0
    assert abs(float(pss.scalar_map("log", np.float32([2.0 ** -24]))[0]) + 24 * np.log(2.0)) < 2e-6
    x = np.concatenate([np.linspace(-20.0, 20.0, 2_000_001), np.linspace(-1e-3, 1e-3, 200_001), np.linspace(-85.0, 85.0, 400_001)]).astype(np.float32)
    x64 = x.astype(np.float64)
    worst_sp = float(_ulp_error(pss.scalar_map("softplus", x), np.maximum(x64, 0) + np.log1p(np.exp(-np.abs(x64)))).max())
    print("largest error in ulp: log", worst_log, "softplus", worst_sp)
    assert worst_log <= 1.0 and worst_sp <= 3.0, (worst_log, worst_sp)
    big = np.float32([100.0, 1e10, 3e38])
    assert np.array_equal(pss.scalar_map("softplus", big), big)
    assert np.all(pss.scalar_map("softplus", -big) > 0) and np.all(pss.scalar_map("softplus", -big) < 1e-37)
    assert pss.scalar_map("softplus", np.float32([0.0]))[0] == np.float32(np.log(2.0))


@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
def test_the_normal_generator(seed):
    """2^20 draws (4 096 keys x 64 blocks x 4): mean, variance and excess kurtosis within 5 standard errors of their sampling
    distributions, lag-1 and cross-block correlation within 5 / 1024, every draw finite and |n| <= 5.78 = sqrt(48 ln 2)."""
    blocks = np.stack([pss.normals((k % 64, k // 64, 3 * k, k % 4), 0, 64, seed) for k in range(4096)]).reshape(4096, 64, 4)
    n = blocks.reshape(-1).astype(np.float64)
    N = n.size
    assert N == 2 ** 20 and np.all(np.isfinite(n)) and np.abs(n).max() <= 5.78
    mean, var = n.mean(), n.var()
    kurt = ((n - mean) ** 4).mean() / var ** 2 - 3.0
    z = (n - mean) / np.sqrt(var)
    lag1 = float((z[:-1] * z[1:]).mean())
    zb = (blocks.astype(np.float64) - mean) / np.sqrt(var)
    cross = float((zb[:, :-1, :] * zb[:, 1:, :]).mean())
    print(f"seed {seed:#x}: mean {mean:.2e} var-1 {var - 1:.2e} kurt {kurt:.2e} lag1 {lag1:.2e} cross-block {cross:.2e}")
    assert abs(mean) <= 5 / 1024 and abs(var - 1) <= 5 * np.sqrt(2 / N) and abs(kurt) <= 5 * np.sqrt(24 / N)
    assert abs(lag1) <= 5 / 1024 and abs(cross) <= 5 / 1024


def _inputs(name, n=16, steps=6, seed=3, track=None):
    """(scan, state, fresh) after a few steps of the deterministic spec's own driving from random starts."""
    env, pol = c_env(track or ("austria" if name == "austria" else "treitlstrasse_v2"), n), PolicySpec(weights(name))
    out = env.reset(mode=ro.RESET_RANDOM, seed=seed)
    st = np.zeros((n, 232), np.float32)
    for _ in range(steps):
        a, st = pol.act_packed(np.asarray(out["lidar"]).reshape(n, 1080), st)
        out = env.step(a, repeat=4)
    return np.asarray(out["lidar"]).reshape(n, 1080).copy(), st, (np.arange(n) % 5 == 3).astype(np.uint8)


@pytest.mark.parametrize("mode", ["deploy", "explore"])
def test_a_cars_draws_do_not_depend_on_the_batch(mode):
    """The normals, the action and the state of (env, slot, episode, step) are the same whether the spec is asked for the car
    alone, for a batch with it, or for the batch in another order; another seed, env, episode, step or slot gives other numbers."""
    scan, state, fresh = _inputs("austria")
    n = len(scan)
    keys = np.stack([np.arange(n) // 2 + 100, np.arange(n) % 3, np.arange(n) * 7, np.arange(n) % 2], 1).astype(np.uint32)
    pol = PolicySampleSpec(weights("austria"), mode, seed=11)
    a, s, d = pol.act_packed(scan, state, fresh, keys, detail=True)
    perm = np.random.default_rng(0).permutation(n)
    a2, s2, d2 = pol.act_packed(scan[perm], state[perm], fresh[perm], keys[perm], detail=True)
    assert np.array_equal(a[perm], a2) and np.array_equal(s[perm], s2) and np.array_equal(d["normals"][perm], d2["normals"])
    for i in (0, 7, n - 1):
        a1, s1, d1 = pol.act_packed(scan[i:i + 1], state[i:i + 1], fresh[i:i + 1], keys[i:i + 1], detail=True)
        assert np.array_equal(a1[0], a[i]) and np.array_equal(s1[0], s[i]) and np.array_equal(d1["normals"][0], d["normals"][i])
    for col in range(4):
        other = keys.copy()
        other[:, col] += 1
        assert not np.any(np.all(pol.act_packed(scan, state, fresh, other, detail=True)[2]["normals"] == d["normals"], 1))
    pol.set_sampling(mode, seed=12)
    assert not np.array_equal(pol.act_packed(scan, state, fresh, keys)[0], a)
    assert np.all(np.abs(a) <= 1.0) and np.array_equal(s[:, 230:], a)
    assert np.all((d["winner"] >= 0) & (d["winner"] < 100)) if mode == "deploy" else np.all(d["winner"] == -1)


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_mode_mean_is_the_deterministic_spec(name):
    scan, state, fresh = _inputs(name)
    want_a, want_s = PolicySpec(weights(name)).act_packed(scan, state, fresh)
    got_a, got_s = PolicySampleSpec(weights(name), "mean").act_packed(scan, state, fresh)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_s, want_s)


def _reference_step(w, scan, state, nrm, mode, amount, dtype):
    """The reference's sampled agent step in `dtype`, fed the normals `nrm` [n, 236] (the spec's layout): RSSM.obs_step with
    stoch = mean + std n (dreamer_policy_port.py:108-114), the tanh-normal actor (:115-124), SampleDist.mode's log-probability
    argmax per car (:126-130, tools.py:301-321) or one sample, additive_gaussian exploration and the clip (models.py:189-202).
    Returns action, stoch, deter, the winner and the gap between the two best scores less _score_gap_bound: positive = the winner is safe."""
    w = {k: np.asarray(w[k], dtype) for k in w.files if k != "source"}
    elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    softplus = lambda x: np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
    nrm = np.asarray(nrm, dtype)
    stoch, deter, prev = (np.asarray(state[:, a:b], dtype) for a, b in ((0, 30), (30, 230), (230, 232)))
    embed = np.clip(np.asarray(scan, dtype), 0.0, 15.0) / dtype(15.0) - dtype(0.5)
    x = elu(np.concatenate([stoch, prev], 1) @ w["img1_w"] + w["img1_b"])
    mx, mh = x @ w["gru_kernel"] + w["gru_bias"][0], deter @ w["gru_recurrent"] + w["gru_bias"][1]
    z, r = sig(mx[:, :200] + mh[:, :200]), sig(mx[:, 200:400] + mh[:, 200:400])
    deter = z * deter + (1 - z) * np.tanh(mx[:, 400:] + r * mh[:, 400:])
    x = elu(np.concatenate([deter, embed], 1) @ w["obs1_w"] + w["obs1_b"])
    x = x @ w["obs2_w"] + w["obs2_b"]
    stoch = x[:, :30] + (softplus(x[:, 30:]) + dtype(0.1)) * nrm[:, :30]
    h = np.concatenate([stoch, deter], 1)
    for i in range(4):
        h = elu(h @ w[f"h{i}_w"] + w[f"h{i}_b"])
    out = h @ w["hout_w"] + w["hout_b"]
    if "hnorm_gamma" in w:
        out = (out - w["hnorm_mean"]) / np.sqrt(w["hnorm_var"] + dtype(1e-3)) * w["hnorm_gamma"] + w["hnorm_beta"]
        mu, sd = out[:, :2], softplus(out[:, 2:]) + dtype(1e-4)
    else:
        mu, sd = dtype(5.0) * np.tanh(out[:, :2] / dtype(5.0)), softplus(out[:, 2:] + dtype(RAW_INIT_STD)) + dtype(1e-4)
    n = len(scan)
    winner, gap = np.full(n, -1), np.full(n, np.inf)
    if mode == "deploy":
        cand = nrm[:, 36:].reshape(n, 100, 2)
        u = mu[:, None] + sd[:, None] * cand
        # log N(u; mu, sd) - log(1 - tanh(u)^2), the bijector's own stable form of the Jacobian
        logp = (-0.5 * cand ** 2 - np.log(sd[:, None]) - 0.5 * np.log(2 * np.pi) - 2.0 * (np.log(2.0) - u - softplus(-2.0 * u))).sum(-1)
        order = np.argsort(-logp, 1, kind="stable")
        winner = order[:, 0]
        pick, second = cand[np.arange(n), winner], cand[np.arange(n), order[:, 1]]
        gap = logp[np.arange(n), order[:, 0]] - logp[np.arange(n), order[:, 1]] - _score_gap_bound(mu, sd, pick, second)
    else:
        pick = nrm[:, 32:34]
    action = np.clip(np.tanh(mu + sd * pick) + dtype(amount) * nrm[:, 34:36], -1.0, 1.0)
    return action, stoch, deter, winner, gap


@pytest.mark.parametrize("mode,amount", [("deploy", 0.0), ("explore", 0.3)])
def test_sampled_modes_are_the_reference_formulas(mode, amount):
    """16 cars, all four checkpoints, 200 agent steps of the spec's own sampled driving on the C oracle with auto-resets; every
    8th step is evaluated from identical inputs and identical normals by the spec, by the float64 restatement and by the same
    restatement in float32.  The spec's largest error against float64 (action, stoch, deter) stays within MARGIN times the
    float32 restatement's own; the winner is the float64 winner wherever float64's two best scores are further apart than
    _score_gap_bound, at most 1 % of the evaluated cars of a run are closer than that - and the float32 restatement, by the same rule, agrees as well.
    Measured: deploy - spec 6.0e-04 / 1.07e-04 / 4.3e-06, float32 3.3e-04 / 7.4e-05 / 3.1e-06, ratios 1.82 / 1.44 / 1.39; of 400
    evaluated cars per checkpoint 1, 1, 3 and 3 lie within the bound, all others have float64's winner; explore - spec
    7.4e-04 / 1.17e-04 / 5.3e-06, float32 3.3e-04 / 6.0e-05 / 5.0e-06, ratios 2.26 / 1.96 / 1.07."""
    n = 16
    err_spec, err_f32 = np.zeros(3), np.zeros(3)
    for name in CHECKPOINTS:
        w = weights(name)
        pol = PolicySampleSpec(w, mode, seed=21, expl_amount=amount)
        env, clock = c_env("austria" if name == "austria" else "treitlstrasse_v2", n), EpisodeClock(n)
        out = env.reset(mode=ro.RESET_RANDOM, seed=2)
        clock.reset()
        st = np.zeros((n, 232), np.float32)
        compared = close = 0
        for k in range(200):
            scan, fresh = np.asarray(out["lidar"]).reshape(n, 1080), np.asarray(out["fresh"]).reshape(n)
            if k:
                clock.step(fresh)
            a, st_new, d = pol.act_packed(scan, st, fresh, clock.keys(), detail=True)
            if k % 8 == 0:
                st_in = st * (fresh == 0)[:, None]
                a64, s64, d64, win64, gap64 = _reference_step(w, scan, st_in, d["normals"], mode, amount, np.float64)
                a32, s32, d32, win32, _ = _reference_step(w, scan, st_in, d["normals"], mode, amount, np.float32)
                sure = gap64 > 0
                if mode == "deploy":
                    compared += n
                    close += int(np.count_nonzero(~sure))
                    assert np.array_equal(d["winner"][sure], win64[sure]), (name, k)
                    assert np.array_equal(win32[sure], win64[sure]), (name, k)
                for j, (got_s, got_p, ref) in enumerate(((a, a32, a64), (st_new[:, :30], s32, s64), (st_new[:, 30:230], d32, d64))):
                    rows = sure if j == 0 else slice(None)           # (another winner is another action: compared where it is the same)
                    err_spec[j] = max(err_spec[j], np.abs(got_s - ref)[rows].max())
                    err_f32[j] = max(err_f32[j], np.abs(got_p - ref)[rows].max())
            st = st_new
            out = env.step(a, repeat=4)
        print(f"{mode} {name}: winners compared {compared - close} of {compared} ({close} within the score error bound)")
        assert close * 100 <= compared
    print(f"{mode}: largest error against float64 (action, stoch, deter): spec", err_spec, "float32", err_f32, "ratio", err_spec / err_f32)
    assert np.all(err_f32 > 0) and np.all(err_spec <= MARGIN * err_f32), (err_spec, err_f32)


def _moments(x):
    """mean, standard deviation and their standard errors, per column."""
    n = len(x)
    m, s = x.mean(0), x.std(0)
    m4 = ((x - m) ** 4).mean(0)
    return m, s, s / np.sqrt(n), np.sqrt(np.maximum(m4 - s ** 4, 0.0) / n) / (2 * s)


@pytest.mark.parametrize("mode", ["deploy", "explore"])
def test_actions_from_one_state_are_distributed_like_the_ports(mode):
    """One (scan, state) pair; 4 096 actions of the spec (4 096 seeds) against 4 096 of the port's own NumPy stream
    (DreamerPolicy(sample=True), for explore with one tanh-normal draw and additive noise 0.3 in its place of the best of 100):
    mean and standard deviation of both components agree within 5 standard errors of the two-sample difference.  The state is one in
    which neither component is saturated (the port's own spread there: 0.11 and 0.08): where tanh(u) sits within a binary32 ulp
    of +-1 the spread is below the format's resolution and the comparison would be one of roundings, not of distributions."""
    scan, state, _ = _inputs("austria")
    scan, state = scan[6:7], state[6:7]          # (the one of the 16 cars whose command the port spreads in both components)
    m = 4096
    w = weights("austria")
    pol = PolicySampleSpec(w, mode, threads=1)
    got = np.empty((m, 2), np.float32)
    for seed in range(m):
        pol.set_sampling(mode, seed=seed)
        got[seed] = pol.act_packed(scan, state, None, np.uint32([[5, 2, 9, 0]]))[0][0]
    port = DreamerPolicy(w, sample=True, seed=123)
    st = dict(stoch=np.repeat(state[:, :30], m, 0), deter=np.repeat(state[:, 30:230], m, 0), action=np.repeat(state[:, 230:], m, 0))
    if mode == "deploy":
        want, _ = port.act(np.repeat(scan, m, 0), st)
    else:
        # the port's posterior sample and actor, then models.py:75-79, 189-202: actor(feat).sample(), Normal(action, 0.3).sample(), clip
        rng = np.random.default_rng(7)
        _, s1 = port.act(np.repeat(scan, m, 0), st)
        h = np.concatenate([s1["stoch"], s1["deter"]], 1).astype(np.float64)
        elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
        for i in range(4):
            h = elu(h @ w[f"h{i}_w"] + w[f"h{i}_b"])
        out = h @ w["hout_w"] + w["hout_b"]
        mu, sd = 5.0 * np.tanh(out[:, :2] / 5.0), np.logaddexp(0.0, out[:, 2:] + RAW_INIT_STD) + 1e-4
        want = np.clip(np.tanh(mu + sd * rng.standard_normal((m, 2))) + 0.3 * rng.standard_normal((m, 2)), -1.0, 1.0)
    gm, gs, gme, gse = _moments(got.astype(np.float64))
    wm, ws, wme, wse = _moments(np.asarray(want, np.float64))
    print(f"{mode}: spec mean {gm} sd {gs}; port mean {wm} sd {ws}; differences in standard errors: mean {np.abs(gm - wm) / np.hypot(gme, wme)}"
          f" sd {np.abs(gs - ws) / np.hypot(gse, wse)}")
    assert np.all(gs > 0) and np.all(np.abs(gm - wm) <= 5 * np.hypot(gme, wme)) and np.all(np.abs(gs - ws) <= 5 * np.hypot(gse, wse))


def _drive_sampled(env, act, n, steps, mode, seed):
    """test_golden_policy.drive for a policy that wants the keys; returns (wall contacts, mean speed after 50 steps, mean laps + progress)."""
    out = env.reset(mode=mode, seed=seed)
    crashes, speeds = 0, []
    for k in range(steps):
        out = env.step(act(k, np.asarray(out["lidar"]).reshape(n, 1080), np.asarray(out["fresh"]).reshape(n)), repeat=4)
        crashes += int(np.count_nonzero(np.asarray(out["wall_collision"])))
        speeds.append(float(np.asarray(out["speed"]).mean()))
    return crashes, float(np.mean(speeds[50:])), float((np.asarray(out["lap"]) + np.asarray(out["progress"])).mean())


@pytest.mark.parametrize("track,mode", [("austria", ro.RESET_GRID), ("austria", ro.RESET_RANDOM), ("columbia", ro.RESET_RANDOM)])
def test_deploy_drives_like_the_ports_sampled_agent(track, mode):
    """Closed loop on the C oracle, 16 cars, 300 agent steps, the austria checkpoint: the spec's deploy mode against the port's
    sample=True on the same starts.  The bar is the port's own result over four of its seeds, with the spread between them as
    the margin: wall contacts <= its most + spread, mean speed and progress >= its least - spread."""
    n, steps = 16, 300
    w = weights("austria")
    ports = []
    for seed in range(4):
        port, box = DreamerPolicy(w, sample=True, seed=seed), {}

        def act_port(k, scan, fresh, port=port, box=box):
            box["s"] = port.initial(n) if k == 0 else box["s"]
            a, box["s"] = port.act(scan, box["s"], reset=(fresh != 0) if k else None)
            return a
        ports.append(_drive_sampled(c_env(track, n), act_port, n, steps, mode, 1))
    pol, clock, box = PolicySampleSpec(w, "deploy", seed=5), EpisodeClock(n), {"s": np.zeros((n, 232), np.float32)}

    def act_spec(k, scan, fresh):
        clock.step(fresh) if k else clock.reset()
        a, box["s"] = pol.act_packed(scan, box["s"], fresh, clock.keys())
        return a
    got = _drive_sampled(c_env(track, n), act_spec, n, steps, mode, 1)
    ports = np.array(ports)
    spread = ports.max(0) - ports.min(0)
    print(f"{track} mode {mode}: spec deploy (contacts, speed, laps) {got}; port sample=True over 4 seeds: min {ports.min(0)} max {ports.max(0)}")
    assert got[0] <= ports[:, 0].max() + spread[0] and got[1] >= ports[:, 1].min() - spread[1] and got[2] >= ports[:, 2].min() - spread[2]


def test_sampling_symbols_and_refusals_without_a_handle(hip_lib):
    from racing_dreamer_amd import _lib as L
    for name in ("rc_policy_set_sampling", "rc_policy_get_sampling"):
        assert name in L.SYMBOLS and hasattr(hip_lib, name)
    assert C.sizeof(L.RcPolicySampling) == 24 and L.POLICY_MODES == {"mean": 0, "deploy": 1, "explore": 2} and L.POLICY_MODE_SAMPLES == 100
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "racecar_hip.h")).read()
    assert "#define RC_POLICY_MODE_SAMPLES 100" in header and "#define RC_ABI_VERSION 3" in header
    s = L.RcPolicySampling(24, 1, 0, 0.0)
    assert hip_lib.rc_policy_set_sampling(None, C.byref(s)) == -1 and hip_lib.rc_policy_get_sampling(None, C.byref(s)) == -1
    from racing_dreamer_amd import build
    assert "rc_policy_sampled_kernel" in build.NO_SPILL_KERNELS and "rc_policy_sampled_kernel" in build.required_kernels("shipped")
