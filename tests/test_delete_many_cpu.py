"""CPU tests of srukf_delete_landmarks: the header declares the call and EXPORTS carries it; its argument refusals need no device;
the launchers are declared once; the 6 x 6 record factorisation and the block covariance each exist as one text that the step-wise getter's kernels and the
batched front call; srukf_delete_landmark has no launch sequence of its own."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def _sources():
    return {fn: _code(fn) for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))}


def _function(txt, head):
    """the text of the function whose definition starts with `head`, to its closing brace in column 0"""
    i = txt.index(head)
    return txt[i:txt.index("\n}\n", i) + 3]


def test_header_declares_the_call_and_exports_carry_it(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+srukf_delete_landmarks\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+K\s*,\s*const\s+int\s*\*\s*ids\s*,\s*double\s*\*\s*records_X6\s*,"
                     r"\s*double\s*\*\s*records_S66\s*,\s*unsigned\s+char\s*\*\s*patches\s*,\s*double\s*\*\s*R\s*,\s*double\s*\*\s*t\s*,\s*double\s*\*\s*px\s*,"
                     r"\s*int\s*\*\s*has_app\s*\)\s*;", txt)
    assert hasattr(lib, "srukf_delete_landmarks") and "srukf_delete_landmarks" in pkg.srukf.EXPORTS
    assert lib.srukf_abi_version() == 6                          # additions only
    assert callable(pkg.srukf.Filter.delete_landmarks)


def test_null_handle_no_landmarks_and_null_ids_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    ids = np.array([0, 1], dtype=np.int32)
    ip = ids.ctypes.data_as(C.POINTER(C.c_int))
    nul = (None,) * 7
    assert lib.srukf_delete_landmarks(None, 2, ip, *nul) == -1
    assert lib.srukf_delete_landmarks(None, 0, ip, *nul) == -1
    assert lib.srukf_delete_landmarks(None, -3, ip, *nul) == -1
    assert lib.srukf_delete_landmarks(None, 2, None, *nul) == -1
    has = np.full(2, 7, dtype=np.int32)
    assert lib.srukf_delete_landmarks(None, 2, ip, None, None, None, None, None, None, has.ctypes.data_as(C.POINTER(C.c_int))) == -1
    assert np.array_equal(has, [7, 7]) and np.array_equal(ids, [0, 1])
    # ... and the refusals with a handle come before the first device call of the body
    m = _code("srukf_map.hip")
    body = _function(m, "static int delete_landmarks_body(")
    i_dev = body.index("hipSetDevice")
    assert body.index("no such landmark") < i_dev and body.index("named twice") < i_dev and body.index("SRUKF_ERR_BAD_ARG") < i_dev
    assert not re.search(r"\bhip[A-Z]\w*\s*\(|\blaunch_\w+\s*\(|map_change_begin", body[:i_dev])
    front = _function(m, "int srukf_delete_landmarks(")
    assert re.search(r"if\s*\(\s*!c\s*\)\s*return\s+SRUKF_ERR_BAD_ARG", front) and re.search(r"K\s*<\s*1\s*\|\|\s*!ids", front)
    assert not re.search(r"\bhip[A-Z]\w*\s*\(|\blaunch_\w+\s*\(", front)


def test_launchers_are_declared_once_in_srukf_launch_h():
    for name in ("launch_lm_records", "launch_appearance_gather", "srukf_launch_block_cov_many"):
        decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
                for _ in re.finditer(r"^void\s+" + name + r"\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
        assert decl == ["srukf_launch.h"], (name, decl)
        defs = [fn for fn, txt in _sources().items() if re.search(r"^void\s+" + name + r"\s*\([^;{]*\)\s*\{", txt, flags=re.M)]
        assert len(defs) == 1, (name, defs)


def test_record_factorisation_and_block_covariance_are_one_text_each():
    src = _sources()
    everything = "".join(src.values())
    # the block covariance: one definition, in srukf_predict.hip; k_block_cov calls it once, for one block or for K (the batched front launches the same kernel)
    pred = src["srukf_predict.hip"]
    assert len(re.findall(r"\bvoid\s+block_cov_body\s*\(", everything)) == 1 and "void block_cov_body" in pred
    assert {fn for fn, txt in src.items() if "block_cov_body" in txt} == {"srukf_predict.hip"}
    assert pred.count("block_cov_body(") == 3                                                          # the definition, k_block_cov, k_image_view
    assert len(re.findall(r"double s\[8\]\[6\]", everything)) == 1                                    # the eight-row trip exists nowhere else
    assert len(re.findall(r"v\[q\+\+\] \+= s\[u\]\[a\] \* s\[u\]\[b\]", everything)) == 2          # block_cov_body's, and landmark_cartesian_body's (the display's own)
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+k_block_cov\s*\(", everything)) == 1
    kbc = _function(pred, re.search(r"__global__[^\n]*\bvoid\s+k_block_cov\s*\(", pred).group(0))
    assert kbc.count("block_cov_body(") == 1 and re.search(r"if\s*\(ids\)\s*\{\s*off = 6 \* ids\[blockIdx\.x\];\s*out \+= 36 \* \(size_t\)blockIdx\.x;\s*\}", kbc)
    assert everything.count("hipLaunchKernelGGL(k_block_cov,") == 2                                    # srukf_launch_block_cov and srukf_launch_block_cov_many
    # the 6 x 6 record factorisation: one definition, two kernels that call it; its pivot rule is written once in the device code
    loop = src["srukf_loop.hip"]
    assert len(re.findall(r"\blm_record_body\s*\(", loop)) == 3 and all("lm_record_body" not in txt for fn, txt in src.items() if fn != "srukf_loop.hip")
    for k in ("k_lm_record", "k_lm_records"):
        assert len(re.findall(r"__global__[^\n]*\bvoid\s+" + k + r"\s*\(", loop)) == 1, k
        kern = _function(loop, re.search(r"__global__[^\n]*\bvoid\s+" + k + r"\s*\(", loop).group(0))
        assert "lm_record_body(" in kern and "sqrt" not in kern and not re.search(r"\bfor\s*\(", kern), k
    assert len(re.findall(r"d = d > eps \? d : eps", loop)) == 1 and len(re.findall(r"const double sjj = sqrt\(d\)", loop)) == 1
    assert len(re.findall(r"\(P66\[6 \* j \+ i\] - q\) / sjj", everything)) == 1
    # the batched front: the getter's two kernels' bodies, the blocks first; plain launches only
    front = _function(loop, "void launch_lm_records(")
    assert front.index("srukf_launch_block_cov_many(") < front.index("hipLaunchKernelGGL(k_lm_records,")
    many = _function(loop, re.search(r"__global__[^\n]*\bvoid\s+k_lm_records\s*\(", loop).group(0))
    gather = _function(src["srukf_map.hip"], re.search(r"__global__[^\n]*\bvoid\s+k_appearance_gather\s*\(", src["srukf_map.hip"]).group(0))
    for dev in (many, kbc, gather):
        assert not re.search(r"\batomic\w*\s*\(", dev) and not re.search(r"\bwhile\s*\(", dev) and "__threadfence" not in dev and "volatile" not in dev
    assert "uint4" in gather and "PT_PATCH_STRIDE % 16 == 0 && PT_TMPL_STRIDE % 16 == 0" in src["srukf_map.hip"]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"srukf_loop\.o:[^\n]*\n\t[^\n]*-ffp-contract=off", mk)                          # the factor rounds as written


def test_delete_landmark_has_no_launch_sequence_of_its_own():
    m = _code("srukf_map.hip")
    one = _function(m, "int srukf_delete_landmark(srukf_ctx* c, int id)")
    assert "delete_landmarks_body(c, \"delete_landmark\", 1, &id, nullptr)" in one
    assert not re.search(r"\blaunch_\w+\s*\(|\bsrukf_launch_\w+\s*\(|map_change_\w+\s*\(|\bhip[A-Z]\w*\s*\(", one)
    many = _function(m, "int srukf_delete_landmarks(")
    assert "delete_landmarks_body(c, \"delete_landmarks\", K, ids," in many
    assert not re.search(r"\blaunch_\w+\s*\(|\bsrukf_launch_\w+\s*\(|map_change_\w+\s*\(", many)
    # the body: one product, one compaction and factorisation, one context swap, one appearance launch; the per-landmark copy loop is gone from it
    body = _function(m, "static int delete_landmarks_body(")
    for call, n in (("srukf_launch_syrk(", 1), ("launch_gather(", 1), ("map_change_factor(", 1), ("map_change_begin(", 1), ("map_change_finish(", 1),
                    ("launch_appearance_gather(", 1), ("launch_lm_records(", 1), ("copy_appearance(", 0)):
        assert body.count(call) == n, (call, body.count(call))
    assert body.index("launch_lm_records(") < body.index("srukf_launch_syrk(") < body.index("launch_gather(") < body.index("map_change_factor(")
    assert m.count("map_change_factor(") == 3 and m.count("launch_sym_permute(") == 1                 # (its definition, add_landmarks, the deletion body)
    add = _function(m, "int srukf_add_landmarks(")
    assert add.count("launch_appearance_gather(") == 1 and "copy_appearance(" not in add
