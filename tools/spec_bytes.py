#!/usr/bin/env python3
"""What bytes do the fit specs give?  One sha256 per (unit, mode, case, output), to compare two trees line for line.  (No GPU.)

    python tools/spec_bytes.py [TESTS_DIR] > listing.txt        # TESTS_DIR: the tests/ of any checkout; default: this one's
    python tools/spec_bytes.py --digest < listing.txt           # the listing in short: one sha256 per (unit, mode) over its lines

For the units fit, reward_fit, actor_fit and action: every case of tests/policy_edge_cases.py in every mode (weights, status, m, v,
grad_features, out - the whole of `spec(unit, make(unit, case), mode)`), and the rows of the three spec test files at N = 97 for three
steps (after each step: loss, grad_norm, skipped, step, grad_flat, grad_features, out; at the end: the weights, m, v) - the actor in
both modes with and without eps, and its forward.  A refactor of the specs leaves the listing as it was."""
import hashlib
import os
import sys

import numpy as np

TESTS = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "--digest" else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
STATUS = ("loss", "grad_norm", "skipped", "step")


def show(unit, mode, case, outputs):
    for k in sorted(outputs):
        a = np.ascontiguousarray(outputs[k], np.float32)
        print(f"{unit:10s} {mode:12s} {case:22s} {k:16s} {a.size:7d} {hashlib.sha256(a.tobytes()).hexdigest()}")


def own_rows(unit, mode, fit, step):
    """Three steps of `fit` through step(), the spec test file's rows."""
    for t in (1, 2, 3):
        got = step()
        show(unit, mode, f"rows97-step{t}", {k: got[k] for k in STATUS + ("grad_flat", "grad_features", "out") if k in got})
    show(unit, mode, "rows97-end", {**fit.weights(), "m": fit.m, "v": fit.v})


def main():
    import policy_edge_cases as pe
    import test_policy_actor_fit_spec as ta
    import test_policy_fit_spec as tf
    import test_policy_reward_fit_spec as tr
    from policy_actor_fit_spec import PolicyActorFitSpec
    from policy_fit_spec import PolicyFitSpec
    from policy_reward_fit_spec import PolicyRewardFitSpec
    for unit in ("fit", "reward_fit", "actor_fit", "action"):
        for case in pe.cases(unit):
            for mode in pe.UNITS[unit]:
                if pe.applies(unit, case, mode):
                    show(unit, mode, case, pe.spec(unit, pe.make(unit, case), mode))
    feat, targets, weight = tf._rows()
    for head in tf.HEADS:
        fit = PolicyFitSpec(tf._critic(), head)
        own_rows("fit", head, fit, lambda: fit.step(feat, targets[head], weight))
    feat, target, weight = tr._rows()
    fit = PolicyRewardFitSpec(tr._head())
    own_rows("reward_fit", "reward", fit, lambda: fit.step(feat, target, weight))
    for mode, with_eps in ta.MODES:
        feat, kw = ta._inputs(mode, with_eps)
        fit = PolicyActorFitSpec(ta._actor())
        name = mode + ("+eps" if with_eps else "")
        show("action", name, "rows97", fit.forward(feat, kw["eps"]))
        own_rows("actor_fit", name, fit, lambda: fit.step(feat, **kw))


def digest(lines):
    groups = {}
    for line in lines:
        groups.setdefault(tuple(line.split()[:2]), []).append(line)
    for (unit, mode), g in groups.items():
        print(f"{unit:10s} {mode:12s} {len(g):5d} lines {hashlib.sha256(''.join(g).encode()).hexdigest()}")
    print(f"{'all':23s} {len(lines):5d} lines {hashlib.sha256(''.join(lines).encode()).hexdigest()}")


if __name__ == "__main__":
    digest(sys.stdin.readlines()) if sys.argv[1:] == ["--digest"] else main()
