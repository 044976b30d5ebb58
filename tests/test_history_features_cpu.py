"""Host side of the resident feature alignment (include/icpmi.h: icpmi_feature_store, icpmi_history_features_add,
icpmi_history_feature_align): the C ABI as the header declares it, the workspace layout against literal sizes, and every
refusal the two entry points decide on the host — before any launch, so no GPU is touched (the pointers are fakes that are
never dereferenced)."""
import ctypes
import os
import re

import numpy as np

from conftest import REPO

NEW_SYMBOLS = ("icpmi_history_features_add", "icpmi_history_feature_align", "icpmi_history_feature_align_workspace_bytes")
FAKE = 4096                                                    # a non-null address that is never dereferenced
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


def fake_history(L, scans=4, rows=8192):
    from icpmi import _lib
    nbytes = L.icpmi_prepared_bytes(rows, scans, 0)
    return _lib.History(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, nbytes, 256, 0.06, 0.3, scans, rows, 10, 1)


def fake_store(**kw):
    from icpmi import _lib
    f = dict(vox=FAKE, curv=FAKE, cnt=FAKE, kp=FAKE, kp_cnt=FAKE, desc=FAKE, desc_len=FAKE, voxel_size=0.2, min_kp_dist=0.3,
             k_curvature=10, top_n=100, k_descriptor=30, kp_stride=104)
    f.update(kw)
    return _lib.FeatureStore(**f)


def test_feature_store_mirror_equals_the_header():
    from icpmi import _lib
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    body = re.search(r"typedef struct icpmi_feature_store \{(.*?)\} icpmi_feature_store;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"([\w\*\s]+?)\s*\b(\w+);", body)
    assert [name for _, name in decl] == [f[0] for f in _lib.FeatureStore._fields_]
    ctype = {"double*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "double": ctypes.c_double, "int32_t": ctypes.c_int32}
    for (kind, name), (fname, ftype) in zip(decl, _lib.FeatureStore._fields_):
        assert ctype["".join(kind.split())] is ftype, (name, kind)
    assert ctypes.sizeof(_lib.FeatureStore) == 7 * 8 + 2 * 8 + 4 * 4
    # the history's own struct is as it was
    assert ctypes.sizeof(_lib.History) == 136


def test_new_entries_are_declared_exported_and_bound():
    import icpmi
    from icpmi import _lib
    path = icpmi.build()
    lib = icpmi.lib()
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(REPO, "include", "icpmi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\(", hdr), name
    assert getattr(lib, "icpmi_history_feature_align").argtypes[0]._type_ is _lib.History
    assert getattr(lib, "icpmi_history_feature_align").argtypes[1]._type_ is _lib.FeatureStore


def test_workspace_bytes_against_literal_values():
    """csrc/features.hip, FtWs with no clouds in front: every array rounded up to 256 bytes, 256 at the end.  5 pairs, top_n 100 (stride 104):
    matches 5 * 104 * 8 = 4160 -> 4352, counts 256; with a start per pair and sources of up to 300 rows the work set adds two
    row arrays of 1500 * 16 -> 24064 each, four small arrays of 256, curvature 12000 -> 12032, keypoints 2080 -> 2304,
    descriptors 133120, and 256 of voxel scratch."""
    import icpmi
    q = icpmi.lib().icpmi_history_feature_align_workspace_bytes
    assert q(5, 300, 100, 0) == 4352 + 256 + 256 == 4864
    assert q(5, 4096, 100, 0) == 4864                                          # no work set: the sources' rows play no part
    assert q(5, 300, 100, 1) == 4864 + 2 * 24064 + 3 * 256 + 12032 + 2304 + 256 + 133120 + 256 + 256 == 201984
    assert q(0, 0, 100, 0) == 256 and q(-1, 300, 100, 0) == 0 and q(5, -1, 100, 1) == 0
    assert q(1, 10, 0, 0) == 256 + 256 + 256 and q(1, 10, 3, 0) == q(1, 10, 8, 0)   # top_n <= 0 or below 8: a stride of 8


def test_features_add_refuses_bad_arguments_on_the_host():
    import icpmi
    from icpmi import _lib
    L = icpmi.lib()
    add = L.icpmi_history_features_add
    off = np.zeros(5, dtype=np.int32)
    offp = off.ctypes.data_as(ctypes.c_void_p)
    h, s = fake_history(L), fake_store()
    B = ctypes.byref
    assert add(B(h), B(s), offp, 0, 0, None) == 0                              # nothing to do
    assert add(None, B(s), offp, 0, 1, None) == ERR_ARG and add(B(h), None, offp, 0, 1, None) == ERR_ARG
    assert add(B(h), B(s), None, 0, 1, None) == ERR_ARG
    assert add(B(_lib.History()), B(s), offp, 0, 1, None) == ERR_ARG
    for field in ("vox", "curv", "cnt", "kp", "kp_cnt", "desc", "desc_len"):
        assert add(B(h), B(fake_store(**{field: None})), offp, 0, 1, None) == ERR_ARG, field
    assert add(B(h), B(s), offp, 3, 2, None) == ERR_ARG                        # beyond the scan capacity
    assert add(B(h), B(s), offp, -1, 1, None) == ERR_ARG
    off[:] = (0, 4000, 8000, 12000, 12000)
    assert add(B(h), B(s), offp, 2, 1, None) == ERR_ARG                        # beyond the row capacity
    off[:] = (0, 4097, 4097, 4097, 4097)
    assert add(B(h), B(s), offp, 0, 1, None) == ERR_UNSUPPORTED                # a scan above 4096 rows
    off[:] = (0, 10, 10, 10, 10)
    assert add(B(h), B(fake_store(k_curvature=32)), offp, 0, 1, None) == ERR_UNSUPPORTED
    assert add(B(h), B(fake_store(k_descriptor=32)), offp, 0, 1, None) == ERR_UNSUPPORTED
    assert add(B(h), B(fake_store(top_n=257, kp_stride=264)), offp, 0, 1, None) == ERR_UNSUPPORTED
    assert add(B(h), B(fake_store(top_n=100, kp_stride=96)), offp, 0, 1, None) == ERR_UNSUPPORTED      # top_n > kp_stride
    assert add(B(h), B(fake_store(voxel_size=0.0)), offp, 0, 1, None) == ERR_ARG


def test_feature_align_refuses_bad_arguments_on_the_host():
    import icpmi
    L = icpmi.lib()
    align = L.icpmi_history_feature_align
    off = np.array([0, 300, 600, 900, 900], dtype=np.int32)
    src = np.zeros(2, dtype=np.int32)
    offp, srcp = off.ctypes.data_as(ctypes.c_void_p), src.ctypes.data_as(ctypes.c_void_p)
    h, s = fake_history(L), fake_store()
    B = ctypes.byref
    need = L.icpmi_history_feature_align_workspace_bytes(2, 300, 100, 1)

    def call(hh=h, ss=s, off_host=offp, pair_src=FAKE, pair_src_host=srcp, pair_tgt=FAKE, n_pairs=2, max_n=300, hyp_idx=None, hyp_u=FAKE,
             n_iter=10, init_in=FAKE, records=FAKE, ws=FAKE, ws_bytes=need):
        return align(B(hh) if hh is not None else None, B(ss) if ss is not None else None, off_host, pair_src, pair_src_host, pair_tgt,
                     n_pairs, max_n, 0.64, hyp_idx, hyp_u, n_iter, 0, 0.5, 3, init_in, FAKE, records, ws, ws_bytes, None)

    assert call(n_pairs=0) == 0                                                # nothing to do
    assert call(n_pairs=0, init_in=None, off_host=None, pair_src_host=None) == 0
    assert call(hh=None) == ERR_ARG and call(ss=None) == ERR_ARG
    for field in ("vox", "cnt", "kp", "kp_cnt", "desc", "desc_len"):
        assert call(ss=fake_store(**{field: None})) == ERR_ARG, field
    for kw in (dict(pair_src=None), dict(pair_tgt=None), dict(records=None), dict(ws=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(off_host=None) == ERR_ARG and call(pair_src_host=None) == ERR_ARG       # a start per pair needs the host mirrors
    assert call(hyp_idx=FAKE) == ERR_ARG and call(hyp_u=None) == ERR_ARG                # exactly one hypothesis table
    assert call(n_pairs=-1) == ERR_ARG and call(max_n=-1) == ERR_ARG
    assert call(ss=fake_store(k_curvature=32)) == ERR_UNSUPPORTED and call(ss=fake_store(k_descriptor=32)) == ERR_UNSUPPORTED
    assert call(ss=fake_store(top_n=257, kp_stride=264)) == ERR_UNSUPPORTED
    assert call(ss=fake_store(top_n=100, kp_stride=96)) == ERR_UNSUPPORTED
    assert call(ss=fake_store(top_n=100, kp_stride=112)) == ERR_ARG                     # not the stride of the work set's tables
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE
    assert call(init_in=None, ws_bytes=L.icpmi_history_feature_align_workspace_bytes(2, 300, 100, 0) - 1) == ERR_WORKSPACE
    src[:] = (0, 4)
    assert call() == ERR_ARG                                                   # a source beyond the scan capacity
    src[:] = (0, -1)
    assert call() == ERR_ARG
    src[:] = (0, 1)
    assert call(max_n=299) == ERR_ARG                                          # a source above max_n rows
    off[:] = (0, 300, 9000, 9000, 9000)
    assert call(max_n=9000, ws_bytes=1 << 30) == ERR_ARG                       # a source beyond the row capacity
