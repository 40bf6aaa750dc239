"""Every owner of device workspaces gives them all back: ``vs_device_bytes_live`` (the process-wide
count of live DevBuf bytes) returns to its value from before an object was made once the object
is closed.

Buffers reached here that the hand-kept release lists of earlier versions had missed:
* flat index, int8 MFMA batch with a device fallback round (``search_device_exact``): the fallback
  round's pre-packed native tile and its counters (Ctx ``qtile_n``, ``gcnt2``, ``drop2``);
* IVF index, mapped MFMA list scan: ``mqidx``, ``mqtile``, ``mcand``, ``mdesc``.
The IVF re-search buffers (``rq`` .. ``rS``) need a query the first pass cannot certify; they are
members like the rest and go with the object's destructor, not exercised here.
"""
import gc

import numpy as np
import pytest

from photo_search_engine_amd import _lib
from photo_search_engine_amd.index import FlatIndex, MultiDeviceFlatIndex

pytestmark = pytest.mark.gpu

D, N, NQ, K = 64, 4096, 16, 10


def _live() -> int:
    gc.collect()  # (handles earlier tests dropped without closing must not close in between)
    return int(_lib.load().vs_device_bytes_live())


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def rows():
    return _unit(N, D, 1), _unit(NQ, D, 2)


def _flat(x, d=D):
    ix = FlatIndex(d, "ip", "bf16")
    ix.add(x)
    ix.set_screen("int8")
    return ix


def test_flat_int8_search_and_device_exact(rows):
    import torch
    x, q = rows
    before = _live()
    ix = _flat(x)
    ix.set_timing(True)
    ix.search(q, K)
    _, kind = ix.timing_fetch()
    assert kind == "mfma_i8"  # the int8 MFMA route ran
    qd = torch.from_numpy(q).cuda()
    I = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    Dd = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
    ix.search_device_exact(qd.data_ptr(), NQ, K, Dd.data_ptr(), I.data_ptr(), None, 0, 0)
    torch.cuda.synchronize()
    _, kind = ix.timing_fetch()
    assert kind == "mfma_i8"
    assert _live() > before
    ix.close()
    assert _live() == before


def test_flat_selector_range_and_probes(rows):
    import torch
    x, q = rows
    before = _live()
    ix = _flat(x)
    sel = ix.selector(np.arange(0, N, 3))
    for mode in ("scan", "overfetch"):
        ix.set_sel_mode(mode)
        ix.search(q, K, sel=sel)
        assert ix.sel_last_stats()["tier"] == mode
    for mode in ("scan", "screen"):
        ix.set_range_mode(mode)
        ix.range_search(q, 0.3)
        assert ix.range_last_stats()["tier"] == mode
    sel.close()
    ix.close()
    assert _live() == before
    # the probes time the direct screens, which need wider rows: bf16 rows of 512 elements
    d2 = 512
    ix = _flat(_unit(N, d2, 3), d2)
    qd = torch.from_numpy(_unit(NQ, d2, 4)).cuda()
    screens = ["native"] + ([] if ix.screen_state()["group_residuals"] else ["int8"])
    for scr in screens:
        assert ix.screen_probe(qd.data_ptr(), NQ, scr, False, 0) > 0.0
        ms, stamps = ix.k1_probe(qd.data_ptr(), NQ, scr, "full", False, 2, 0)
        assert len(ms) == 2 and stamps.shape[0] == 2
    ix.close()
    assert _live() == before


def test_ivf_mapped_mfma_list_scan(rows):
    from photo_search_engine_amd.ivf import IVFFlatIndex
    x, _ = rows
    q = _unit(32, D, 5)
    before = _live()
    ix = IVFFlatIndex(D, 2, "ip", "bf16")
    ix.set_centroids(x[:2])
    ix.add(x)
    ix.set_scan("mfma")
    ix.search(q, K, 2)  # 32 queries probe both lists: the mapped MFMA list scan
    assert ix.last_mfma_lists > 0
    assert _live() > before
    ix.close()
    assert _live() == before


def test_hnsw_search(rows):
    from oracle import hnsw_oracle as H
    from photo_search_engine_amd.hnsw import HNSWGraph
    x, q = rows
    before = _live()
    ix = FlatIndex(D, "ip", "f32")
    ix.add(x[:600])
    hg = HNSWGraph(ix, H.layered_knn_graph(x[:600], 4, "ip", seed=1))
    hg.search(q, K, 32)
    assert _live() > before
    hg.close()
    ix.close()
    assert _live() == before


def test_multi_device_single_device(rows):
    x, q = rows
    before = _live()
    mx = MultiDeviceFlatIndex(D, "ip", "bf16", devices=(0,))
    mx.add(x)
    mx.search(q, K)
    assert _live() > before
    mx.close()
    assert _live() == before
