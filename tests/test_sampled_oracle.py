"""tests/sampled_oracle.py against the reference's transcripts (tests/golden/sampled), and its samplers' law. CPU."""
import glob
import os

import numpy as np
import pytest

import sampled_oracle as so
from oracle.oracle import load_transcript

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "sampled", "ezs_*.npz")))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_replays_reference_bit_for_bit(path):
    g = load_transcript(path)
    got = so.replay(g, lambda k: so.glibc_draws(g["seeds"][k]))
    for name in ("req_x", "req_y", "req_len", "req_vtp", "out_dist"):
        assert np.array_equal(got[name], g[name]), name
    assert np.abs(got["out_values"] - g["out_values"]).max() <= 1e-5


def test_continuous_sampler_is_standard_normal():
    z = np.concatenate([so.gaussian_z(12345, L, 7, 64, 3).ravel() for L in range(200)])
    n = 64 * 3 * 200
    assert z.size == n and abs(z.mean()) <= 5 / np.sqrt(n)  # se(mean) = 1 / sqrt(n)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n)                 # se(var) = sqrt(2 / n) for a normal


def test_discrete_sampler_first_slot_follows_p():
    logits = np.array([0.5, -1.0, 2.0, 0.0, -0.3], np.float32)
    p, n = so.discrete_probs(logits).astype(np.float64), 4000
    draw = so.philox_sampler(99, 2, False)
    freq = np.bincount([draw(L, 3, logits)[0] for L in range(n)], minlength=5) / n
    assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / n))
