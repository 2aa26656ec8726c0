"""bench.py's harness logic (argument handling, JSON contract, roofline / cpu_baseline
objects, the plain run against --full) exercised at toy size on the emulator build; the numbers mean nothing here."""
import json

import bench


def test_bench_json_contract(emu_lib, capsys):
    out = bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "4096", "--cols", "8", "--cpu-sample-n", "4096", "--prewarm-seconds", "0.05", "--side-scale", "0.04",
                      "--full"], lib=emu_lib)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f64"
    assert d["vs_baseline"] is None and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0
    assert out["value"] > 0
    assert d["check"]["iters"] == 4 and "resumed" in d["config"]["timed_region"] and d["single_call"]["value"] > 0
    assert d["roofline"]["traffic"] is None            # no PMC passes of this build
    ops = d["extras"]["operators"]                   # the one-pass iteration with non-diagonal Hessians, timed beside the headline
    assert "error" not in ops and ops["tridiagonal_one_pass_ms"] > 0 and ops["diagonal_plus_rank4_one_pass_ms"] > 0


def test_bench_plain_run_measures_the_headline_only(emu_lib, tmp_path, capsys, monkeypatch):
    """Without --full the run sets up, warms up, times the steps, dumps and prints: the contract keys and the figures of the timed steps, none
    of the side measurements (CPU baseline, extras, further windows, single call, matvecs) -- and the timed steps and their outputs are the
    ones a --full run makes."""
    import numpy as np

    def refused(*a, **k):
        raise AssertionError("side measurement in a plain run")
    common = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--rows", "5000", "--cols", "6", "--prewarm-seconds", "0.02", "--cpu-sample-n", "5000",
              "--side-scale", "0.04"]
    with monkeypatch.context() as mp:
        mp.setattr(bench, "cpu_baseline", refused)
        mp.setattr(bench, "extras", refused)
        bench.main([*common, "--dump-outputs", str(tmp_path / "plain")], lib=emu_lib)
    d = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "kernels", "check"):
        assert key in d, key
    for key in ("cpu_baseline", "extras", "further_windows_iters_per_s", "single_call", "matvec", "first_allocation"):
        assert key not in d, key
    assert d["steps"] == 3 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["check"]["iters"] == 5
    bench.main([*common, "--full", "--dump-outputs", str(tmp_path / "full")], lib=emu_lib)
    f = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for key in ("cpu_baseline", "extras", "further_windows_iters_per_s", "single_call", "matvec", "first_allocation"):
        assert key in f, key
    assert f["check"] == d["check"]
    for name in ("x", "x_rows", "nr", "iters"):
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy"))


def test_bench_dump_outputs(emu_lib, tmp_path, capsys):
    """--dump-outputs DIR: the timed call's x, nr and iteration count after its last step, float64; --steps sets the number of timed
    steps; the same arguments give the same outputs."""
    import numpy as np
    common = ["--gpus", "1", "--warmup", "2", "--rows", "5000", "--cols", "6", "--prewarm-seconds", "0.02", "--no-cpu-baseline", "--no-extras"]
    got = []
    for k, d in ((3, tmp_path / "a"), (3, tmp_path / "b"), (5, tmp_path / "c")):
        bench.main([*common, "--steps", str(k), "--dump-outputs", str(d)], lib=emu_lib)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["steps"] == k and line["ms_per_step"] > 0 and line["check"]["iters"] == 2 + k
        f = {p.stem: np.load(p) for p in d.glob("*.npy")}
        assert sorted(f) == ["iters", "nr", "x", "x_rows"] and all(a.dtype == np.float64 for a in f.values())
        assert f["iters"][0] == 2 + k and f["nr"][0] == line["check"]["nr"]
        np.testing.assert_array_equal(f["x_rows"], np.arange(5000))
        assert abs(np.linalg.norm(f["x"]) - line["check"]["x_norm"]) <= 1e-14 * line["check"]["x_norm"]    # (summation order)
        got.append(f)
    for key in got[0]:
        np.testing.assert_array_equal(got[0][key], got[1][key])
    assert not np.array_equal(got[0]["x"], got[2]["x"])
    # entry by entry against the same solve made here through the library (bench.py's generators: basis seed 1 orthonormalised,
    # A = diag(5.5 + 4.5 u) seed 3, b seed 4; 2 warmup iterations, then 3 more resumed) and downloaded independently
    import lfpsqp_jl_amd as L
    ctx = L.Context(0, emu_lib)
    n, m = 5000, 6
    Z = ctx.matrix(n, m).hash_fill(1, 0, n, 1.0)
    L.orthonormalize_(Z, n_global=n)
    A, U, b, x = L.DiagOperator(0.0, ctx.vector(n).hash_fill(3, 0, 4.5, 5.5)), L.DeviceBasis(Z), ctx.vector(n).hash_fill(4, 0), ctx.vector(n)
    work = L.ProjCGWork(ctx, n, m)
    L.projcg_(x, None, A, U, b, None, tol=1e-300, maxit=2, work=work, n_global=n, want_lambda=False)
    it, _ = L.projcg_(x, None, A, U, b, None, tol=1e-300, maxit=3, work=work, n_global=n, want_lambda=False, resume=True)
    assert it == 5
    np.testing.assert_allclose(got[0]["x"], x.download(), rtol=1e-12, atol=1e-14)
    ctx.close()


def test_bench_dump_outputs_samples_large_x(tmp_path):
    """Above bench.DUMP_ROWS rows x is written as a fixed sorted sample of its rows (the same for every run), within 64 MB in all."""
    import numpy as np

    class _Vec:
        n = 3_000_000

        def download(self):
            return np.arange(self.n, dtype=np.float64) * 0.5

    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), _Vec(), 7, 1e-3, _Vec.n, 0, 0, None)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert a["x"].size == bench.DUMP_ROWS and np.all(np.diff(a["x_rows"]) > 0)
    np.testing.assert_array_equal(a["x"], a["x_rows"] * 0.5)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key])
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 64 << 20


def test_bench_two_ranks_as_the_driver_launches_it(emu_lib, tmp_path):
    """`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`: row-sharded workload, one
    all-reduce per iteration (gloo here, RCCL on the GPUs), barrier-bracketed timing, rank 0 prints the one line;
    the solve is the same as the single-rank one."""
    import os
    import socket
    import subprocess
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    EMU_LIB = os.path.join(ROOT, "tests", "emu", "_build", "liblfpsqp_emu.so")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    common = ["--steps", "4", "--warmup", "1", "--rows", "9000", "--cols", "8", "--no-cpu-baseline", "--prewarm-seconds", "0.2", "--lib", EMU_LIB]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--comm", "host-gloo", "--device", "0", *common,
           "--dump-outputs", str(tmp_path / "two")]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                   # rank 0 only
    d2 = json.loads(lines[0])
    assert d2["n_gpus"] == 2 and d2["scaling"] == "strong" and d2["config"]["parallelism"] == "row-sharded x2"
    assert "extras" not in d2 and d2["value"] > 0
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-extras", *common, "--dump-outputs", str(tmp_path / "one")],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][0])
    assert d1["check"]["iters"] == d2["check"]["iters"] == 5        # 1 warmup + 4 timed iterations of one solve
    assert abs(d1["check"]["x_norm"] - d2["check"]["x_norm"]) <= 1e-10 * d1["check"]["x_norm"]
    # --dump-outputs over two uneven shards (rank 0 gathers): the same rows and, to rounding, the same x as the one-rank dump
    import numpy as np
    f1, f2 = ({k: np.load(d / f"{k}.npy") for k in ("x", "x_rows", "nr", "iters")} for d in (tmp_path / "one", tmp_path / "two"))
    assert d2["config"]["rows_per_gpu"] != 4500                     # (the shards are uneven)
    np.testing.assert_array_equal(f2["x_rows"], np.arange(9000))
    np.testing.assert_array_equal(f1["x_rows"], f2["x_rows"])
    assert f1["iters"][0] == f2["iters"][0] == 5
    np.testing.assert_allclose(f2["x"], f1["x"], rtol=1e-10, atol=1e-13)


def test_bench_starts_its_own_ranks_when_called_without_a_launcher(emu_lib):
    """`python bench.py --gpus 4` with no torch.distributed.run around it (the form the driver uses for --gpus 1): the parent, which has
    touched no GPU, starts the ranks as one child, relays rank 0's line and the exit code.  Four ranks over the library's one-shot
    peer-to-peer all-reduce (named explicitly, then picked by --comm auto: the emulator build has no RCCL behind it, so that probe is skipped and recorded);
    the solve is the single-rank one."""
    import os
    import subprocess
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    EMU_LIB = os.path.join(ROOT, "tests", "emu", "_build", "liblfpsqp_emu.so")
    common = ["--steps", "4", "--warmup", "1", "--rows", "19000", "--cols", "8", "--no-cpu-baseline", "--prewarm-seconds", "0.1", "--lib", EMU_LIB]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    got = {}
    for comm in ("p2p", "auto"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--comm", comm, "--device", "0", *common], cwd=ROOT,
                             capture_output=True, text=True, timeout=900, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["n_gpus"] == 4 and d["config"]["parallelism"] == "row-sharded x4" and d["config"]["rows_per_gpu"] == 6144
        assert "p2p" in d["config"]["comm"] and "fine-grained" in d["config"]["comm"]
        pr = d["config"]["comm_probe"]
        assert pr["chosen"] == "p2p" and pr["p2p"]["ok"] and pr["p2p"]["mailbox_memory"] == "fine-grained" and pr["p2p"]["us_per_allreduce"] > 0
        if comm == "auto":
            assert pr["ranks_share_a_gpu"] and pr["rccl"]["ok"] is False
        got[comm] = d
    assert got["p2p"]["check"] == got["auto"]["check"]                       # fixed rank order: bit for bit
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-extras", *common], cwd=ROOT,
                         capture_output=True, text=True, timeout=600, env=env)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][0])
    assert d1["check"]["iters"] == got["p2p"]["check"]["iters"] == 5
    assert abs(d1["check"]["x_norm"] - got["p2p"]["check"]["x_norm"]) <= 1e-10 * d1["check"]["x_norm"]
    # a launcher whose WORLD_SIZE contradicts --gpus is an error, not a silent 1-rank run
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", *common], cwd=ROOT, capture_output=True, text=True,
                         timeout=120, env=dict(env, WORLD_SIZE="1", RANK="0"))
    assert bad.returncode != 0 and "WORLD_SIZE" in bad.stderr
