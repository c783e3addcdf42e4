"""The switch table of srukf_debug_set (srukf_debug.hip, k_switches), checked without a device: the listed keys are the documented ones, and every process-wide
key stores what its row says.  No filter is created: the process-wide keys take a NULL context, and setting one only stores an integer.

Every process-wide value is saved first and put back at the end, so that GPU tests running later in the same process meet the defaults.  One key cannot be put
back: "head_fold_free" refuses values below 1, its default 0 among them.  The values it accepts are therefore set in a child process (this file run as a script),
which never touches a device either."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
BATCH_GROUPS_MAX = 4                                            # SRUKF_BATCH_GROUPS_MAX
INT_MAX = 2**31 - 1

ONOFF, RAW, FROM0 = ("onoff", 0, 1), ("clamp", -INT_MAX - 1, INT_MAX), ("clamp", 0, INT_MAX)
PROCESS = {
    "gmw_persist": ONOFF, "gmw_fused": ONOFF, "rank_fused": ONOFF, "rank_fold": ONOFF, "graphs": ONOFF, "rank_aware": ONOFF,
    "mem_split": RAW, "head_fold_free": ("refuse", 1, INT_MAX),
    "batch_split": ONOFF, "batch_k128": ONOFF, "batch_xcd": ONOFF,
    "batch_wide": ONOFF, "timing": ONOFF, "fold_force": ONOFF, "pivot_relay": ONOFF,
    "batch_groups": ("refuse", 0, BATCH_GROUPS_MAX), "shared_tenants": ("refuse", 2, 8),
    "fold_head": FROM0, "ctx_keep": FROM0, "exact_rl": RAW,
}
FILTER = {
    "use_graph": ONOFF, "pxy2": ONOFF, "nullskip": ONOFF, "head_fold": ONOFF, "tail_fuse": ONOFF, "table_perm": ONOFF, "f32_fuse": ONOFF, "split_record": ONOFF,
    "gain_fold": ONOFF, "null_canon": ONOFF, "mixed_rank": ONOFF, "mixed_f64_robot": ONOFF, "mixed_bf16": ONOFF, "step_fast": ONOFF, "step_spin": ONOFF,
    "step_fuse_export": ONOFF, "view_auto": ONOFF,
    "split_fold": ("clamp", 0, 2), "step_early": ("clamp", 0, 2), "fused_motion": ("clamp", 0, 2), "mixed_null_ppm": FROM0,
}
DEFAULTS = {k: 1 for k in list(PROCESS) + list(FILTER)}
DEFAULTS.update(timing=0, fold_force=0, split_record=0, gain_fold=0, mixed_bf16=0, fold_head=0, head_fold_free=0, batch_groups=0, shared_tenants=2, ctx_keep=24,
                fused_motion=2, step_early=2, split_fold=1, mixed_null_ppm=1)
VALUES = (-5, 0, 1, 2, 99)


def stored(rule, x):
    """What a row stores for x; None: x is refused and nothing is stored."""
    kind, lo, hi = rule
    if kind == "onoff":
        return 1 if x else 0
    if lo <= x <= hi:
        return x
    return None if kind == "refuse" else min(max(x, lo), hi)


def check_process_key(srukf, key, values):
    """set(key, x) for each x: the read-back is what the row says, and no other key's value moved."""
    lib = srukf.load_library()
    for x in values:
        before = srukf.debug_switches()
        rc = lib.srukf_debug_set(None, key.encode(), x)
        after = srukf.debug_switches()
        want = stored(PROCESS[key], x)
        assert rc == (BAD_ARG if want is None else 0), (key, x, rc)
        assert after[key][2] == (before[key][2] if want is None else want), (key, x, after[key])
        assert {k: v for k, v in after.items() if k != key} == {k: v for k, v in before.items() if k != key}, (key, x)


@pytest.fixture()
def restored(pkg):
    srukf = pkg.srukf
    saved = {k: v for k, (per_filter, _, v) in srukf.debug_switches().items() if not per_filter}
    try:
        yield srukf
    finally:
        for k, v in saved.items():
            if srukf.debug_switches()[k][2] != v:
                srukf.debug_set_global(k, v)
        assert {k: v[2] for k, v in srukf.debug_switches().items() if not v[0]} == saved


def test_listed_keys_are_the_documented_ones(pkg):
    sw = pkg.srukf.debug_switches()
    assert {k for k, v in sw.items() if not v[0]} == set(PROCESS)
    assert {k for k, v in sw.items() if v[0]} == set(FILTER)
    assert {k: v[1] for k, v in sw.items()} == DEFAULTS
    for k, (per_filter, default, value) in sw.items():
        if per_filter:
            assert value == default, k                          # no filter: the default
    # every key appears in quotes in the comment above srukf_debug_set
    txt = open(os.path.join(ROOT, "include", "srukf.h")).read()
    end = txt.index("srukf_debug_set(srukf_ctx* ctx")
    comment = txt[txt.rindex("/*", 0, end):end]
    assert "Process-wide keys" in comment and "Per-context keys" in comment
    quoted = set(re.findall(r'"([a-z_0-9]+)"', comment))
    assert not set(sw) - quoted, sorted(set(sw) - quoted)
    # the table has an end
    lib = pkg.srukf.load_library()
    assert lib.srukf_debug_switch_at(None, len(sw), None, None, None, None) == BAD_ARG
    assert lib.srukf_debug_switch_at(None, -1, None, None, None, None) == BAD_ARG
    assert lib.srukf_debug_switch_at(None, 0, None, None, None, None) == 0


def test_keys_that_need_a_filter_refuse_a_null_context(restored):
    lib = restored.load_library()
    before = restored.debug_switches()
    for key in list(FILTER) + ["no_such_key", ""]:
        for x in VALUES:
            assert lib.srukf_debug_set(None, key.encode(), x) == BAD_ARG, key
    assert lib.srukf_debug_set(None, None, 1) == BAD_ARG
    assert restored.debug_switches() == before


@pytest.mark.parametrize("key", sorted(PROCESS))
def test_process_wide_key_stores_what_its_row_says(restored, key):
    if key != "head_fold_free":
        check_process_key(restored, key, VALUES)
        return
    # what it refuses, here; what it accepts, where it does not stay behind
    check_process_key(restored, key, [x for x in VALUES if stored(PROCESS[key], x) is None])
    assert [x for x in VALUES if stored(PROCESS[key], x) is None] == [-5, 0]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), key], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checked head_fold_free [1, 2, 99]" in r.stdout, r.stdout + r.stderr


def test_examples(restored):
    lib, sw = restored.load_library(), restored.debug_switches

    def put(key, x):
        return lib.srukf_debug_set(None, key.encode(), x)
    assert put("ctx_keep", -5) == 0 and sw()["ctx_keep"][2] == 0
    was = sw()["batch_groups"][2]
    assert put("batch_groups", 99) == BAD_ARG and sw()["batch_groups"][2] == was
    assert put("shared_tenants", 1) == BAD_ARG
    assert put("mem_split", 2) == 0 and sw()["mem_split"][2] == 2
    assert put("exact_rl", 2) == 0 and sw()["exact_rl"][2] == 2
    assert put("timing", 99) == 0 and sw()["timing"][2] == 1
    was = sw()["head_fold_free"][2]
    assert put("head_fold_free", 0) == BAD_ARG and sw()["head_fold_free"][2] == was
    assert lib.srukf_gmw_get_pivot_relay() == sw()["pivot_relay"][2]
    assert put("pivot_relay", 0) == 0 and lib.srukf_gmw_get_pivot_relay() == 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    key = sys.argv[1]
    values = [x for x in VALUES if stored(PROCESS[key], x) is not None]
    check_process_key(ge.load_package().srukf, key, values)
    print("checked", key, values)
