"""Builds liblzmcts.so in-tree for gfx950 (hipcc). Invoked by __graft_entry__.build()."""
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("LZM_OFFLOAD_ARCH", "gfx950")
# -ffp-contract=off: no fused multiply-add anywhere in the tree kernels, so every fp32
# expression rounds like the reference's SSE build; division and sqrt stay IEEE (HIP default).
# -fno-slp-vectorize: no v_pk_fma_f32 pairing in the fused search's dense layers — its operand
# pairs cost ~3 v_mov each (measured: ~370 -> ~75 moves per network step).
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared", "-Wall",
         f"--offload-arch={ARCH}"]
SOURCES = [os.path.join(HERE, "csrc", "lzm_kernels.hip")]
# Translation units compiled with the packed-f32 VALU forms (v_pk_add / mul / fma_f32) switched off in the target,
# then linked in: the Connect4 AlphaZero kernels, whose trees and network bits are pinned to a plain f32 restatement.
# A guard, not a tuning: the present compiler emits none of these forms there either way (the device assembly is
# the same with and without the feature). It cannot go on lzm_kernels.hip, which uses packed FMAs on purpose
# (profiles/EXPERIMENTS.md, "packed FMA") and whose kernels change with it; hence the separate unit.
# The one-launch Stochastic MuZero and Sampled EfficientZero searches' kernels (lzm_search_stoch_mlp.hip,
# lzm_search_sampled_mlp.hip) and the Stochastic MuZero conv step (lzm_smz_conv.hip) are built the same way: they
# use no packed form, and the feature keeps it so. The Gomoku AlphaZero kernels (lzm_az_gomoku.hip) are pinned like
# the Connect4 ones and built like them, and so are the 9 x 9 / 15 x 15 ones (lzm_az_gomoku_n.hip) and their
# split-fp16 network (lzm_az_gomoku_n_split.hip, a unit of its own so that the f32 kernels' unit compiles as before).
# tools/build_variant.sh builds the same units.
NO_PK_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
NO_PK_SOURCES = [os.path.join(HERE, "csrc", n) for n in ("lzm_az_c4.hip", "lzm_az_gomoku.hip", "lzm_az_gomoku_n.hip",
                                                         "lzm_az_gomoku_n_split.hip",
                                                         "lzm_search_stoch_mlp.hip", "lzm_search_sampled_mlp.hip",
                                                         "lzm_smz_conv.hip")]
DEPS = SOURCES + NO_PK_SOURCES + sorted(glob.glob(os.path.join(HERE, "csrc", "*.h")) +
                        glob.glob(os.path.join(HERE, "csrc", "*.inc"))) + [os.path.join(REPO, "include", "lzmcts.h")]
OUT = os.path.join(HERE, "liblzmcts.so")


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return OUT
    with tempfile.TemporaryDirectory(prefix="lzm_build_") as tmp:
        objs = []
        for src in NO_PK_SOURCES:
            obj = os.path.join(tmp, os.path.splitext(os.path.basename(src))[0] + ".o")
            cmd = [HIPCC] + [f for f in FLAGS if f != "-shared"] + NO_PK_F32 + ["-c", "-o", obj, src]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
            objs.append(obj)
        cmd = [HIPCC] + FLAGS + ["-o", OUT] + objs + SOURCES  # objects first: hipcc puts -x hip before a .hip file
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
