"""The owning wrappers of csrc/vs_internal.h (DevBuf, HostBuf, DevEvent, PinnedPair) under the
address and undefined-behaviour sanitizers: tests/host/devbuf_moves.cpp is a stand-alone program
(HIP allocations replaced by counting host stubs) built for the host and run on the CPU."""
import os
import subprocess

from photo_search_engine_amd import build

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "devbuf_moves.cpp")


def test_owning_wrappers_move_and_count_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devbuf_moves")
    cc = subprocess.run([build._hipcc(), "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                         "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "devbuf_moves: ok" in run.stdout
