"""The launch log's host side, without a GPU: the two C-ABI calls on an empty table, and LDPC_HIP_LAUNCH_LOG=<file> -- read when the library is
loaded, one block per process appended when it is unloaded (no HIP call there: it works in a process that never touched a device)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_log_is_off_and_empty_by_default():
    from ldpc_amd import _lib
    from ldpc_amd.engine import launch_log
    lib = _lib.load()
    assert lib.ldpc_hip_debug_launch_log_read(None, 0) == 1  # the terminating NUL of an empty text
    with launch_log() as log:
        pass
    assert log == {}


def test_environment_variable_appends_one_block_per_process(tmp_path):
    out = tmp_path / "launches.txt"
    env = dict(os.environ, LDPC_HIP_LAUNCH_LOG=str(out), PYTHONPATH=ROOT)
    pids = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", "import os; from ldpc_amd import _lib; _lib.load(); print(os.getpid())"], env=env, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        pids.append(int(r.stdout.split()[-1]))
    assert out.read_text().splitlines() == [f"# pid {p}" for p in pids]
