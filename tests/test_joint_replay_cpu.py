"""The joint update as a mode of the staged replay: what the header, the Python binding and the C++ host agree on without a GPU
(the device side: tests/test_gpu_joint_replay.py)."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_name_the_mode(pkg):
    hdr = open(os.path.join(ROOT, "include", "srukf.h")).read()
    enum = re.search(r"typedef enum srukf_update_mode \{([^}]*)\}", hdr).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(SRUKF_UPDATE_\w+)\s*=\s*(\d+)", enum)}
    assert vals == {"SRUKF_UPDATE_SEQUENTIAL": 0, "SRUKF_UPDATE_BATCHED": 1, "SRUKF_UPDATE_JOINT": 2}
    assert re.search(r"#define SRUKF_ABI_VERSION 6\b", hdr)                         # an addition: the version stays
    assert re.search(r"int\s+srukf_prepare_frames_mode\(srukf_ctx\* ctx, int count, int mode\);", hdr)
    assert "Not part of the staged replay" not in hdr
    s = pkg.srukf
    assert (s.UPDATE_SEQUENTIAL, s.UPDATE_BATCHED, s.UPDATE_JOINT) == (0, 1, 2)
    assert "srukf_prepare_frames_mode" in s.EXPORTS
    sig = inspect.signature(s.Filter.prepare_frames)
    assert list(sig.parameters) == ["self", "count", "mode"] and sig.parameters["mode"].default == s.UPDATE_BATCHED


def test_step_bench_offers_the_replay_mode(pkg):
    exe = os.path.join(ROOT, "cv-monoslam_amd", "cslam_step_bench.bin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert out.returncode == 2 and "mode=<capi|facade|assoc|replay>" in out.stderr
