"""bench.py's N-rank launch on CPU: `python bench.py --gpus 2` without a
launcher starts torch.distributed.run with 2 ranks as a child process, the
ranks join one process group (gloo here; RCCL on the GPU node), time a
barrier-bracketed region, take the max over ranks and rank 0 prints one JSON
line with n_gpus = 2 (--launch-check: the plumbing without GPU work)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n):
    env = dict(os.environ, MTTS_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--launch-check",
                        "--steps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_launches_two_ranks():
    rec = _run(2)
    assert rec["n_gpus"] == 2 and rec["allreduce_ok"] and rec["steps"] == 3 and rec["warmup"] == 1
    # the N > 1 line explains itself: backward time, the all-reduce time left
    # exposed after it, and the bucket layout (bench.py dp_breakdown)
    dp = rec["dp"]
    assert dp["backward_ms"] >= 0 and dp["allreduce_exposed_ms"] >= 0 and dp["steps"] == 3
    assert dp["buckets"] >= 2 and len(dp["bucket_MB"]) == dp["buckets"] and dp["grad_MB"] > 0
    assert dp["comm_dtype"] == "float32" and dp["reduce_op"] in ("avg", "sum+scale")


def test_bench_single_rank_needs_no_launcher():
    assert _run(1)["n_gpus"] == 1


def test_dump_outputs_writes_a_fixed_float32_sample(tmp_path):
    """--dump-outputs: loss, logits whole; parameters and gradients whole up to
    DUMP_PER_TENSOR elements, else the same DUMP_PER_TENSOR seeded elements in
    every call (so two builds can be compared output for output)."""
    import numpy as np
    import torch
    import bench
    k = bench.DUMP_PER_TENSOR
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(3 * k + 5, generator=g)), torch.nn.Parameter(torch.randn(7, 3, generator=g)),
              torch.nn.Parameter(torch.randn(4, generator=g))]
    params[0].grad = torch.randn(3 * k + 5, generator=g)
    params[1].grad = torch.randn(7, 3, generator=g)          # params[2]: unused, no gradient
    loss = torch.tensor(1.25, dtype=torch.float64)
    logits = torch.randn(2, 5, 10, generator=g).to(torch.bfloat16)
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, logits, params)
        assert sorted(os.listdir(tmp_path / d)) == ["grads_sample.npy", "logits.npy", "loss.npy", "params_sample.npy"]
        got.append({n: np.load(tmp_path / d / (n + ".npy")) for n in ("loss", "logits", "grads_sample", "params_sample")})
    a, b = got
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert a["loss"].tolist() == [1.25] and np.array_equal(a["logits"], logits.float().numpy())
    assert a["params_sample"].shape == a["grads_sample"].shape == (k + 21 + 4,)
    # the small tensors are whole and in order; the large one's sample holds its own elements, pairwise with its grads
    assert np.array_equal(a["params_sample"][k:k + 21], params[1].detach().reshape(-1).numpy())
    assert np.array_equal(a["grads_sample"][k:k + 21], params[1].grad.reshape(-1).numpy())
    assert np.array_equal(a["grads_sample"][k + 21:], np.zeros(4, np.float32))
    lookup = {float(p): float(gr) for p, gr in zip(params[0].detach().tolist(), params[0].grad.tolist())}
    assert all(lookup[float(p)] == float(gr) for p, gr in zip(a["params_sample"][:k], a["grads_sample"][:k]))
