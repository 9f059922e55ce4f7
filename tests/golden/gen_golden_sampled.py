"""Generate the Sampled EfficientZero golden transcripts tests/golden/sampled/ezs_*.npz.

Test infrastructure only. Compiles the REFERENCE tree module
``lzero/mcts/ctree/ctree_sampled_efficientzero/ezs_tree.pyx`` from the reference checkout (environment variable
LZ_REFERENCE, default /root/reference) into ``oracle/_ref/`` (git-ignored) with the recipe of
``oracle/build_ref.sh`` and of gen_golden_stochastic.py (``oracle/ref_time_hook.c`` under
``-Wl,--wrap=gettimeofday``, so the srand(tv_usec) of every batch_traverse takes a chosen seed). It then drives the
module as ``SampledEfficientZeroMCTSCtree.search`` (``lzero/mcts/tree_search/mcts_ctree_sampled.py:133-232``) does,
the network replaced by tables that are a function of (simulation, root): the reference samples its actions from a
wall-clock seed, and with such tables they never reach a tree decision.

The script prints the libm entry points the compiled module imports (``nm -D``); tests/sampled_oracle.py restates
cucb_score with the float forms it finds there.

    python tests/golden/gen_golden_sampled.py
"""
import ctypes
import os
import subprocess
import sys
import sysconfig

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_DIR = os.path.join(REPO, "oracle", "_ref")
OUT_DIR = os.path.join(HERE, "sampled")
sys.path[:0] = [REPO, os.path.dirname(HERE)]
import sampled_oracle as so  # noqa: E402  (the shared table builder and constants)


def build_reference():
    ref = os.environ.get("LZ_REFERENCE", "/root/reference")
    src = os.path.join(ref, "lzero", "mcts", "ctree", "ctree_sampled_efficientzero")
    if not os.path.isdir(src):
        sys.exit(f"{src} not present: the reference checkout is needed to regenerate the goldens")
    bld = os.path.join(REF_DIR, "build")
    os.makedirs(bld, exist_ok=True)
    out = os.path.join(REF_DIR, "ezs_tree" + sysconfig.get_config_var("EXT_SUFFIX"))
    cpp, hook = os.path.join(bld, "ezs_tree.cpp"), os.path.join(bld, "ref_time_hook.o")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", os.path.join(REPO, "oracle", "ref_time_hook.c"), "-o", hook])
    subprocess.check_call(["cython", "--cplus", "-3", "-I", src, "-o", cpp, os.path.join(src, "ezs_tree.pyx")])
    subprocess.check_call(["g++", "-DNDEBUG", "-g0", "-fwrapv", "-O2", "-fPIC", "-shared", "-std=c++11", "-w",
                           "-I" + sysconfig.get_paths()["include"], "-I" + src, cpp, hook,
                           "-Wl,--wrap=gettimeofday", "-o", out])
    syms = subprocess.check_output(["nm", "-D", "--undefined-only", out], text=True).split()
    print("libm imports:", sorted(s.split("@")[0] for s in syms if s.split("@")[0] in
                                  ("exp", "expf", "log", "logf", "sqrt", "sqrtf", "pow", "powf", "tanh", "tanhf")))
    return out


CASES = {  # every search is longer than the LSTM horizon, so is_reset is crossed; K = 1: a path as deep as S
    "ezs_cont_b5_s24_k3": dict(B=5, S=24, K=3, dim=2, cont=True, seed=1),
    "ezs_cont_2p_b8_s25_k20": dict(B=8, S=25, K=20, dim=3, cont=True, players=2, seed=2),
    "ezs_cont_deep_b4_s12_k1": dict(B=4, S=12, K=1, dim=1, cont=True, seed=3),
    "ezs_cont_zero_b5_s24_k3": dict(B=5, S=24, K=3, dim=2, cont=True, net="zero", seed=4),
    "ezs_disc_b5_s24_k3": dict(B=5, S=24, K=3, dim=6, cont=False, seed=5),
    "ezs_disc_2p_zero_b8_s25_k20": dict(B=8, S=25, K=20, dim=24, cont=False, net="zero", players=2, seed=6),
    "ezs_disc_deep_b4_s12_k1": dict(B=4, S=12, K=1, dim=4, cont=False, seed=7),
}


def gen_case(c, tree, lib):
    d = so.scripted(**c)
    B, S, K, to_play = c["B"], c["S"], c["K"], d["to_play"].tolist()
    roots = tree.Roots(B, [[-1] for _ in range(B)], c["dim"], K, c["cont"])
    roots.prepare_no_noise(d["root_vp"].tolist(), d["root_policy"].tolist(), list(to_play))
    mms = tree.MinMaxStatsList(B)
    mms.set_delta(so.VDM)
    req = {k: np.zeros((S, B), np.int32) for k in ("x", "y", "vtp", "len")}
    for k in range(S):
        lib.oracle_set_usec(int(d["seeds"][k]))
        res = tree.ResultsWrapper(num=B)
        x, y, _, vtp = tree.batch_traverse(roots, *so.PB_C, so.DISC, mms, res, list(to_play), c["cont"])
        lens = res.get_search_len()
        for name, v in zip(req, (x, y, vtp, lens)):
            req[name][k] = np.asarray(v, np.int32)
        tree.batch_backpropagate(k + 1, so.DISC, d["resp_vp"][k].tolist(), d["resp_value"][k].tolist(),
                                 d["resp_policy"][k].tolist(), mms, res, [int(l % so.HORIZON == 0) for l in lens],
                                 list(vtp))
    d.update({"req_" + k: v for k, v in req.items()})
    dist = roots.get_distributions()
    assert all(len(r) == K for r in dist) and all(len(r) == K for r in roots.get_sampled_actions())
    d.update(out_dist=np.array(dist, np.int32), out_values=np.array(roots.get_values(), np.float32))
    return d


def main():
    so_path = build_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    sys.path.insert(0, REF_DIR)
    import ezs_tree  # noqa: E402  (reference build, test infrastructure)
    lib = ctypes.CDLL(so_path)
    lib.oracle_set_usec.argtypes = [ctypes.c_long]
    for name, c in CASES.items():
        d = gen_case(c, ezs_tree, lib)
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, **d)
        print(f"{name}: max search_len {d['req_len'].max()} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
