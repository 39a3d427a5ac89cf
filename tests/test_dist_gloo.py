"""World-size-2 checks of the N>1 path on the gloo backend (CPU): the path shards along the batch with no
data-path collective; what has to hold across ranks is (a) batch sharding gives the same
result as the un-sharded op, (b) parameter gradients summed over shards equal the full-batch gradients
(what DDP's all-reduce does around the module), (c) bench.py's max-over-ranks timing and aggregation.
The device op has no CPU path, so the oracle stands in for it here -- this exercises the host logic only."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import bench
    from oracle import cca_oracle as O
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        assert bench.dist_env() == (rank, world, rank)
        # identical full problem on every rank (same seed), each rank computes its own batch shard
        torch.manual_seed(0)
        B, C, H, W = 4, 16, 6, 5
        conv = {n: torch.nn.Conv2d(C, o, 1) for n, o in (("query_conv", C // 8), ("key_conv", C // 8), ("value_conv", C))}
        params = {"gamma": torch.full((1,), 0.5)}
        for n, m in conv.items():
            params[n + ".weight"], params[n + ".bias"] = m.weight.detach(), m.bias.detach()
        x, dy = torch.randn(B, C, H, W), torch.randn(B, C, H, W)
        lo, hi = rank * B // world, (rank + 1) * B // world
        y_s, dx_s, g_s = O.cca_module_forward_backward(x[lo:hi], params, dy[lo:hi])
        # (b) sum the parameter gradients over ranks (DDP averages; the sum is the un-sharded gradient)
        for n in sorted(g_s):
            dist.all_reduce(g_s[n], op=dist.ReduceOp.SUM)
        # (a) gather the shards
        ys = [torch.empty_like(y_s) for _ in range(world)]
        dist.all_gather(ys, y_s)
        y_full, dx_full, g_full = O.cca_module_forward_backward(x, params, dy)
        assert torch.allclose(torch.cat(ys), y_full, atol=1e-5)
        assert torch.allclose(dx_s, dx_full[lo:hi], atol=1e-5)
        for n in g_full:
            assert torch.allclose(g_s[n], g_full[n], rtol=1e-4, atol=1e-4), n
        # (c) timing reduction + whole-job aggregation used by bench.py
        t = bench.max_over_ranks(0.5 + rank, torch.device("cpu"), world)
        assert t == pytest.approx(0.5 + (world - 1))
        v = bench.aggregate_value(1_000_000_000, 10, world, t)
        assert v == pytest.approx(world * 10 / t)
        assert bench.shard_seed(1234, rank) == 1234 + rank
        out.put((rank, "ok"))
    except Exception as e:  # surface the failure in the parent
        out.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_world_size_two_batch_sharding_on_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
    assert res == {0: "ok", 1: "ok"}, res


def _bench_env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    return env


def _run_bench(args, env):
    import subprocess
    import sys
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=600)


def test_bench_gpus_2_self_spawns_two_ranks_on_gloo():
    """VERDICT r1 item 2 / ADVICE: ``bench.py --gpus 2`` with no launcher must really run two ranks (here on gloo
    with the oracle stand-in workload) and say so; the N=1 line keeps its shape."""
    import json
    common = ["--steps", "2", "--warmup", "1", "--batch", "2", "--channels", "16", "--height", "6", "--width", "5",
              "--prewarm-s", "0", "--backend", "gloo", "--workload-factory", "bench_standin:factory"]
    p = _run_bench(["--gpus", "2", "--allreduce-grads"] + common, _bench_env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout                              # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 4 and out["scaling"] == "weak"
    assert "(B,16,6,5)" in out["metric"] and "all-reduce" in out["config"]["parallelism"]
    # the first N-GPU run must be diagnosable -- one entry per rank (its own time, host, pid, device) and the
    # collective library on the line
    assert [r["rank"] for r in out["per_rank"]] == [0, 1] and len({r["pid"] for r in out["per_rank"]}) == 2
    assert all(r["ms_per_step"] > 0 and r["device"] == "cpu" for r in out["per_rank"])
    assert max(r["ms_per_step"] for r in out["per_rank"]) <= out["ms_per_step"] * 1.001 + 1e-3
    assert out["collective_library"]["backend"] == "gloo"
    one = _run_bench(["--gpus", "1"] + common, _bench_env())
    assert one.returncode == 0, one.stderr[-2000:]
    o1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert o1["n_gpus"] == 1 and o1["algorithmic_bytes_per_step_per_gpu"] == out["algorithmic_bytes_per_step_per_gpu"]
    assert set(o1) == set(out) and len(o1["per_rank"]) == 1


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    env = _bench_env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = _run_bench(["--gpus", "4", "--backend", "gloo", "--workload-factory", "bench_standin:factory"], env)
    assert p.returncode != 0 and "WORLD_SIZE=1 but --gpus 4" in p.stderr


def test_bench_refuses_more_gpus_than_devices():
    p = _run_bench(["--gpus", "8"], _bench_env())                 # nccl backend, no HIP device in this container
    assert p.returncode != 0 and "refusing" in p.stderr


def test_bench_dump_outputs_is_the_last_timed_steps_result(tmp_path):
    """``--dump-outputs DIR``: what the timed path computed, one float32 ``<name>.npy`` per output, the same from run to run
    (seeded inputs); ``--steps`` is the number of timed steps (no pre-run here: warm-up + timed = every step taken)."""
    import numpy as np
    import bench
    import bench_standin
    from oracle import cca_oracle as O
    made = []

    def factory(*a):
        made.append(bench_standin.factory(*a))
        return made[-1]

    common = ["--gpus", "1", "--warmup", "2", "--batch", "2", "--channels", "16", "--height", "6", "--width", "5",
              "--prewarm-s", "0", "--backend", "gloo"]
    dumps = []
    for run, steps in enumerate((3, 5)):
        d = tmp_path / f"run{run}"
        out = bench.main(common + ["--steps", str(steps), "--dump-outputs", str(d)], workload_factory=factory)
        assert out["steps"] == steps and made[-1].steps == 2 + steps
        assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in ("y", "A", "dq", "dk", "dv", "dgamma"))
        assert set(out["dumped_outputs"]["arrays"]) == {"y", "A", "dq", "dk", "dv", "dgamma"}
        dumps.append({n: np.load(d / (n + ".npy")) for n in ("y", "A", "dq", "dk", "dv", "dgamma")})
    wl = made[-1]
    y, A = O.cca_core_forward(wl.q, wl.k, wl.v, wl.x, wl.gamma)
    g = O.cca_core_backward(wl.dy, wl.q, wl.k, wl.v, A, wl.gamma)
    want = {"y": y, "A": A, **{n: g[n] for n in ("dq", "dk", "dv", "dgamma")}}
    for n, t in want.items():
        assert dumps[0][n].dtype == np.float32 and dumps[0][n].shape == tuple(t.shape), n
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
        assert np.array_equal(dumps[1][n], t.numpy()), n
    # an output above the sample size: a fixed, seeded sample of its elements, the same positions every time
    big = {"v": torch.arange(3000, dtype=torch.float32).reshape(30, 100)}
    d1, d2 = bench.dump_outputs(big, str(tmp_path / "s1"), sample=256), bench.dump_outputs(big, str(tmp_path / "s2"), sample=256)
    s1, s2 = np.load(tmp_path / "s1" / "v.npy"), np.load(tmp_path / "s2" / "v.npy")
    assert d1 == {**d2, "dir": d1["dir"]} and d1["arrays"]["v"]["sampled"] and 200 < s1.size <= 256
    assert s1.dtype == np.float32 and np.array_equal(s1, s2) and np.all(np.diff(s1) > 0)
    assert np.isin(s1, big["v"].float().numpy()).all()


def test_bench_refuses_zero_steps():
    p = _run_bench(["--steps", "0", "--backend", "gloo", "--workload-factory", "bench_standin:factory"], _bench_env())
    assert p.returncode != 0 and "--steps" in p.stderr
