"""The synthetic assets of the drop-in tests (tests/test_dropin_cpu.py, tests/test_dropin_gpu.py): a diffusers-layout checkpoint and a
VITON-HD-layout test set, written by the tools of this repository in child processes.  No GPU and no package import."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_assets(tmp_path, size=256, n=2):
    ck, dd = str(tmp_path / "ckpt"), str(tmp_path / "data")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    for cmd in ([sys.executable, os.path.join(ROOT, "tools", "make_synth_ckpt.py"), ck],
                [sys.executable, os.path.join(ROOT, "tools", "make_synth_vitonhd.py"), dd, "--n", str(n), "--width", str(size), "--height", str(size)]):
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return ck, dd
