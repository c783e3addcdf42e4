"""The per-filter rows of srukf_debug_set's switch table on a real filter (the process-wide rows: tests/test_switches_cpu.py, which also holds the table's
expected content).  No frame runs: N = 8 is the smallest map the suite builds, and a switch is a field of the filter it is set on."""
import pytest

from test_switches_cpu import DEFAULTS, FILTER, stored

pytestmark = pytest.mark.gpu


def test_every_per_filter_key_reaches_its_own_field_of_its_own_filter(srukf, synth):
    p = synth.scene_params()
    sc = synth.make_scene(8, 1, seed=0, p=p)
    f = srukf.Filter(8, p)
    f.set_state(sc["X0"], sc["S0"])
    g = None
    try:
        start = srukf.debug_switches(f)
        assert {k for k, v in start.items() if v[0]} == set(FILTER)
        assert all(v[2] == v[1] == DEFAULTS[k] for k, v in start.items() if v[0]), start
        g = srukf.Filter(8, p)                                 # created meanwhile: nothing set on f may show here
        for key in FILTER:
            for x in (-1, 0, 1, 3):
                before = srukf.debug_switches(f)
                f.debug_set(key, x)                            # raises unless SRUKF_OK
                after = srukf.debug_switches(f)
                assert after[key][2] == stored(FILTER[key], x), (key, x, after[key])
                assert {k: v for k, v in after.items() if k != key} == {k: v for k, v in before.items() if k != key}, (key, x)
                assert srukf.debug_switches(g) == start, (key, x)
            assert f.debug_get("use_graph") == srukf.debug_switches(f)["use_graph"][2]
        for key in FILTER:
            f.debug_set(key, DEFAULTS[key])
        assert srukf.debug_switches(f) == start
        with pytest.raises(srukf.SrukfError) as e:
            f.debug_set("no_such_key", 1)
        assert e.value.rc == -1 and "srukf_debug_set: unknown key no_such_key" in str(e.value)
    finally:
        f.close()
        if g is not None:
            g.close()
