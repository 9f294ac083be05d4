"""bench.py's launch contract, checked without a GPU: `--gpus N` must agree with WORLD_SIZE when a launcher set it, and a plain
`python bench.py --gpus N` (N > 1) must start N rank processes itself through torch.distributed.run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_gpus_flag_must_match_world_size():
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "4"], cwd=ROOT, env=_env(WORLD_SIZE="2", RANK="0"), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 2 and "WORLD_SIZE=2" in p.stderr


def test_plain_launch_builds_a_torchrun_command(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3"])
    monkeypatch.delenv("MASTER_PORT", raising=False)
    assert bench.launch_ranks(8) == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "8", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_secondary_measurements_need_full():
    """A plain run only times the steps: asking for one of the legs without --full is an error, before any work is done."""
    for opt in ("--cpu-rounds", "--scan-leg-rounds", "--dense-leg-rounds", "--dense-job", "--map-leg-repeats"):
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", opt, "1"], cwd=ROOT, env=_env(), capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 2 and "runs only with --full" in p.stderr, (opt, p.stderr)
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "0", "--dump-outputs", "out"], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps >= 1" in p.stderr


def _paf(rows):
    return "".join("r%07d\t%d\t%d\t%d\t%s\tr%07d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (r[0], r[1], r[2], r[3], "+" if r[4] else "-", *r[5:])
                   for r in rows).encode()


def test_dump_outputs_holds_the_whole_paf(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    rows = [(0, 10000, 49, 958, 1, 9739, 10000, 2130, 3039, 182, 0, 255), (0, 10000, 49, 958, 0, 44713, 10000, -297, 628, 182, 0, 255),
            (3, 9000, 0, 1000, 1, 1, 10000, 9000, 10000, 60, 0, 255)]
    assert bench.paf_table(_paf(rows)).tolist() == [list(r) for r in rows]
    ignore = np.array([0, 1, 0, 0, 1], dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), _paf(rows), ignore)
    got = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert got["paf_lines_per_query_read"].dtype == np.float64 and got["paf_lines_per_query_read"].tolist() == [2, 0, 0, 1, 0]
    assert got["paf_column_sums"].tolist() == np.array(rows).sum(axis=0).tolist()
    assert got["paf_rows"].dtype == np.float64 and got["paf_rows"].tolist() == [list(r) for r in rows]
    assert got["ignore_flags"].dtype == np.float32 and got["ignore_flags"].tolist() == [0, 1, 0, 0, 1]
    bench.dump_outputs(str(tmp_path / "empty"), b"", ignore)
    assert np.load(str(tmp_path / "empty" / "paf_rows.npy")).shape == (0, 12)


def test_dump_outputs_samples_the_same_rows_every_time(tmp_path, monkeypatch):
    """Over DUMP_SAMPLE_ROWS lines the rows are a fixed, seeded sample in PAF order; the per-read counts and sums stay whole."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 50)
    rows = [(i // 10, 10000, i, i + 900, i % 2, 39 - i // 10, 10000, 2 * i, 2 * i + 900, 100, 0, 255) for i in range(400)]
    paf = _paf(rows)
    ignore = np.zeros(40, dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), paf, ignore)
    bench.dump_outputs(str(tmp_path / "b"), paf, ignore)
    a, b = np.load(str(tmp_path / "a" / "paf_rows.npy")), np.load(str(tmp_path / "b" / "paf_rows.npy"))
    assert a.shape == (50, 12) and (a == b).all()
    idx = [rows.index(tuple(int(x) for x in r)) for r in a]
    assert idx == sorted(idx)
    assert np.load(str(tmp_path / "a" / "paf_lines_per_query_read.npy")).sum() == 400
