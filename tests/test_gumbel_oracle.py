"""The host restatement of the Gumbel MuZero tree (tests/gumbel_oracle.py) replays every reference
transcript tests/golden/gumbel/gmz_*.npz bit for bit: the requests of every simulation and all five outputs."""
import glob
import os

import numpy as np
import pytest

import gumbel_oracle as go

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(go.GOLDEN, "gmz_*.npz"))
               if not p.endswith("gmz_tables.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_cases_present():
    assert len(CASES) >= 10
    for name in ("gmz_b8_s25_a2", "gmz_b4_s16_a6", "gmz_b3_s50_a18"):
        assert name in CASES


def test_fallback_case_reaches_fallback():
    assert int(np.load(os.path.join(go.GOLDEN, "gmz_b4_s16_a6.npz"))["fallbacks"][0]) > 0


@pytest.mark.parametrize("name", CASES)
def test_replay(name):
    g = np.load(os.path.join(go.GOLDEN, name + ".npz"))
    t, req = go.replay(g)
    for k, gk in (("x", "req_x"), ("y", "req_y"), ("a", "req_a"), ("vtp", "req_vtp"), ("len", "req_len")):
        assert np.array_equal(req[k], g[gk]), k
    A = int(g["meta"][2])
    disc = g["consts"][0]
    assert np.array_equal(go.pad(t.distributions(), A), g["out_dist"])
    assert np.array_equal(go.pad(t.trajectories(), g["out_traj"].shape[1])[:, :g["out_traj"].shape[1]], g["out_traj"])
    assert np.array_equal(bits(t.values()), bits(g["out_values"]))
    assert np.array_equal(bits(t.children_values(disc)), bits(g["out_children_values"]))
    assert np.array_equal(bits(t.policies(disc)), bits(g["out_policies"]))


def test_considered_visits_rows():
    tabs = np.load(os.path.join(go.GOLDEN, "gmz_tables.npz"))
    for m, S in tabs["ms"]:
        assert go.considered_visits(int(m), int(S)) == tabs[f"row_{m}_{S}"].tolist(), (m, S)
