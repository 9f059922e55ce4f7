"""CPU: bench.py's multi-rank launch (`--gpus N` without torchrun) and the push rules.

`python bench.py --gpus 2 --dry-run` must start two rank processes itself (RANK / WORLD_SIZE set,
rendezvous on 127.0.0.1), they join a gloo group, and rank 0 prints one JSON line naming both
ranks. The GPU path uses the same launcher with RCCL (`--gpus` used to be ignored).
"""
import json
import os
import subprocess
import sys
import tarfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=180):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_gpus2_launches_two_ranks():
    line = _run(["--gpus", "2", "--dry-run"])
    assert line["dry_run"] is True and line["n_gpus"] == 2
    assert [r["rank"] for r in line["ranks"]] == [0, 1]
    assert [r["local_rank"] for r in line["ranks"]] == [0, 1]


def test_bench_gpus1_is_one_process():
    line = _run(["--dry-run"])
    assert line["n_gpus"] == 1 and [r["rank"] for r in line["ranks"]] == [0]


def test_dump_outputs_formats_and_sample(tmp_path, monkeypatch):
    """--dump-outputs: tensors only, floats as float32 / float64, integers as float64 (exact); an array over
    its share of the byte budget is stored as the same sorted sample every time; other ranks get a suffix"""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    out = {"distributions": torch.arange(12, dtype=torch.int32).reshape(4, 3), "skipped": None,
           "values": torch.linspace(0, 1, 4, dtype=torch.float64), "half": torch.ones(5, dtype=torch.float16)}
    info = bench.dump_outputs(str(tmp_path / "a"), out, 0)
    assert sorted(info) == ["distributions", "half", "values"]
    d = np.load(tmp_path / "a" / "distributions.npy")
    assert d.dtype == np.float64 and np.array_equal(d, np.arange(12).reshape(4, 3))
    assert np.load(tmp_path / "a" / "values.npy").dtype == np.float64
    assert np.load(tmp_path / "a" / "half.npy").dtype == np.float32
    bench.dump_outputs(str(tmp_path / "a"), out, 1)
    assert (tmp_path / "a" / "values.rank1.npy").exists()
    # 16 data bytes per array beside its header allowance: 2 float64 / 4 float32 elements
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * (16 + bench.NPY_HEADER_BYTES))
    bench.dump_outputs(str(tmp_path / "b"), out, 0)
    bench.dump_outputs(str(tmp_path / "c"), out, 0)
    for name, n in (("distributions", 2), ("values", 2), ("half", 4)):
        b, c = np.load(tmp_path / "b" / f"{name}.npy"), np.load(tmp_path / "c" / f"{name}.npy")
        assert b.shape == (n,) and np.array_equal(b, c)
    full = np.arange(12, dtype=np.float64)
    assert np.all(np.diff(np.load(tmp_path / "b" / "distributions.npy")) > 0)  # sorted picks of the flat array
    assert np.isin(np.load(tmp_path / "b" / "distributions.npy"), full).all()
    # the files together, headers included, stay within the budget
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= bench.DUMP_MAX_BYTES
    assert bench.DUMP_MAX_BYTES <= 64e6


def test_sum_returns_adds_counts_and_keeps_descriptions():
    """a timed collect region with several trajectory returns reports their sums (bench.sum_returns)"""
    sys.path.insert(0, REPO)
    import bench
    a = {k: 1 for k in bench.TRAJ_SUMMED}
    a.update(collective_ms=0.25, frame_dtype="uint8", world=1, backend="nccl", mode="gather(dst=0)")
    b = dict(a, episodes_received=5, payload_bytes_received=700, collective_ms=0.5)
    out = bench.sum_returns([a, b, a])
    assert out["returns"] == 3 and out["episodes_received"] == 7 and out["payload_bytes_received"] == 702
    assert out["collective_ms"] == 1.0 and out["frame_dtype"] == "uint8" and out["mode"] == "gather(dst=0)"
    none = dict(a, collective_ms=None, wire_bytes_sent=None, wire_bytes_received=None)  # (no process group)
    out = bench.sum_returns([none, none])
    assert out["collective_ms"] is None and out["wire_bytes_sent"] is None and out["rows_received"] == 2


def test_reference_build_does_not_travel(tmp_path):
    """.gpurunignore keeps oracle/_ref (the reference's ctree compiled here) out of every push:
    checked with tar's own --exclude-from semantics on a scratch tree of the same layout."""
    pats = [ln.strip() for ln in open(os.path.join(REPO, ".gpurunignore")) if ln.strip() and not ln.startswith("#")]
    assert "./oracle/_ref" in pats
    root = tmp_path / "repo"
    for rel in ("oracle/_ref/mz_tree.cpython-310-x86_64-linux-gnu.so", "oracle/liblzoracle.so",
                "lightzero_amd/liblzmcts.so", "oracle/lz_oracle.c"):
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_bytes(b"x")
    out = tmp_path / "push.tar"
    subprocess.check_call(["tar", "-cf", str(out), "--exclude-from", os.path.join(REPO, ".gpurunignore"), "."],
                          cwd=root)
    names = tarfile.open(out).getnames()
    assert not any("_ref" in n for n in names), names
    for keep in ("./oracle/liblzoracle.so", "./lightzero_amd/liblzmcts.so", "./oracle/lz_oracle.c"):
        assert keep in names, (keep, names)
