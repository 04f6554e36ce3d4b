"""The gallery's selection rule (NumPy oracle), FaceGallery bookkeeping on a CPU stub of the kernels, argument checks of the C ABI,
and the metrics of identify_efm.py on hand-made CSVs — no GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from improving_face_recognition_performance_using_triplet_loss_amd import _lib, gallery as gallery_mod
from tests import gallery_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_threshold_ties_by_index_and_fill():
    s = np.array([[0.5, 0.9, 0.5, 0.1, 0.9, 0.3]])
    sc, ix, lb = O.topk(s, 4, sim_th=0.3)
    assert ix.tolist() == [[1, 4, 0, 2]] and sc.tolist() == [[0.9, 0.9, 0.5, 0.5]] and lb.tolist() == [[-1] * 4]
    sc, ix, _ = O.topk(s, 6, sim_th=0.4)
    assert ix.tolist() == [[1, 4, 0, 2, -1, -1]] and sc[0, 4:].tolist() == [NINF, NINF]
    sc, ix, _ = O.topk(s, 3, sim_th=0.95)
    assert ix.tolist() == [[-1, -1, -1]]


def test_sim_th_is_inclusive_and_zero_query_matches_nothing():
    g = np.eye(3)
    s = O.scores(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), g)
    sc, ix, _ = O.topk(s, 2, sim_th=1.0)
    assert ix.tolist() == [[0, -1], [-1, -1]]


def test_identity_dedup_keeps_best_row_of_each_label():
    s = np.array([[0.9, 0.8, 0.95, 0.7, 0.6, 0.95]])
    labels = [3, 3, 5, 7, 7, 3]
    sc, ix, lb = O.topk(s, 3, labels=labels)
    assert lb.tolist() == [[5, 3, 7]] and ix.tolist() == [[2, 5, 3]]   # 0.95 tie between rows 2 (label 5) and 5 (label 3)
    sc, ix, lb = O.topk(s, 5, labels=labels, sim_th=0.75)
    assert lb.tolist() == [[5, 3, -1, -1, -1]]


@pytest.mark.parametrize("by_label", [False, True])
def test_chunk_tops_merge_to_the_whole(by_label):
    rng = np.random.default_rng(1)
    s = np.round(rng.uniform(-1, 1, size=(7, 300)), 2)   # rounding makes many exact ties
    labels = rng.integers(0, 25, size=300)
    for k in (1, 5, 32):
        whole = O.topk(s, k, 0.1, labels if by_label else None)
        cuts = [0, 13, 14, 150, 300]
        parts = [O.topk(s[:, a:b], k, 0.1, labels[a:b] if by_label else None, row_offset=a) for a, b in zip(cuts[:-1], cuts[1:])]
        got = O.merge(parts, k, by_label)
        for w, g in zip(whole, got):
            assert np.array_equal(w, g)


# ---------------------------------------------------------------------------------------- FaceGallery on a CPU stub
class _Stub:
    """The four ops the gallery calls, in NumPy on CPU tensors: pack normalises, scan takes the oracle's per-chunk top-k."""
    GALLERY_KMAX = 32
    pad32 = staticmethod(lambda c: (c + 31) & ~31)

    def __init__(self):
        self.scans = []
        self.slots = {}

    def gallery_workspace_bytes(self, nq, nslots, k):
        return 16

    def gallery_pack(self, x, dst):
        v = x.double()
        n = v.norm(dim=1, keepdim=True)
        v = torch.where(n > 0, v / n, torch.zeros_like(v))
        dst.zero_()
        dst[:, :x.shape[1]] = v.to(dst.dtype)

    def gallery_scan(self, query, g, n, labels, row_offset, k, sim_th, ws, slot):
        self.scans.append((n, row_offset, slot, labels is not None))
        s = O.scores(query.numpy(), g[:n, :query.shape[1]].double().numpy())
        self.slots[slot] = O.topk(s, k, sim_th, labels.numpy() if labels is not None else None, row_offset)

    def gallery_merge(self, ws, nslots, nq, k, by_label):
        sc, ix, lb = O.merge([self.slots[i] for i in range(nslots)], k, by_label)
        return torch.tensor(sc, dtype=torch.float32), torch.tensor(ix, dtype=torch.int32), torch.tensor(lb, dtype=torch.int32)


@pytest.fixture
def stub(monkeypatch):
    st = _Stub()
    monkeypatch.setattr(gallery_mod, "ops", st)
    return st


def test_capacity_grows_geometrically_and_splits_into_chunks(stub):
    g = gallery_mod.FaceGallery(20, dtype="f32", device="cpu", chunk_rows=3000)
    assert len(g) == 0 and g.capacity == 0 and g.ld == 32
    rng = np.random.default_rng(0)
    g.enroll(torch.tensor(rng.standard_normal((700, 20)), dtype=torch.float32), np.arange(700) % 9)
    assert len(g) == 700 and g.capacity == 1024
    g.enroll(torch.tensor(rng.standard_normal((700, 20)), dtype=torch.float32), np.arange(700) % 9)
    assert len(g) == 1400 and [c.shape[0] for c, _ in g._chunks] == [2048]
    g.enroll(torch.tensor(rng.standard_normal((5000, 20)), dtype=torch.float32), np.arange(5000) % 9)
    assert len(g) == 6400 and [u for _, u in g.chunks] == [3000, 3000, 400]
    assert [c.shape[0] for c, _ in g._chunks] == [3000, 3000, 1024]
    assert g.labels.shape == (6400,) and g.labels[1400:1405].tolist() == [0, 1, 2, 3, 4]
    # the rows are stored unit-norm with zero pad columns
    f = g._chunks[0][0][:10]
    assert torch.allclose(f[:, :20].norm(dim=1), torch.ones(10)) and bool((f[:, 20:] == 0).all())


def test_default_chunks_stay_below_2_gib():
    for dt, es in (("bf16", 2), ("f32", 4)):
        g = gallery_mod.FaceGallery(342, dtype=dt, device="cpu")
        assert g.ld == 352 and g.chunk_rows * 352 * es < 2 ** 31 and (g.chunk_rows + 1) * 352 * es >= 2 ** 31 - 1


def test_search_over_chunks_matches_the_oracle_over_the_whole(stub):
    rng = np.random.default_rng(3)
    feats = rng.standard_normal((2500, 16)).astype(np.float32)
    labels = rng.integers(0, 40, size=2500)
    g = gallery_mod.FaceGallery(16, dtype="f32", device="cpu", chunk_rows=1000)
    g.enroll(torch.tensor(feats[:1200]), labels[:1200])
    g.enroll(torch.tensor(feats[1200:]), labels[1200:])
    q = rng.standard_normal((5, 16)).astype(np.float32)
    stored = g.features().double().numpy()
    for by_id in (False, True):
        stub.scans.clear()
        sc, ix, lb = g.search(torch.tensor(q), k=7, sim_th=0.2, by_identity=by_id)
        assert [(n, off, slot, has) for n, off, slot, has in stub.scans] == [(1000, 0, 0, by_id), (1000, 1000, 1, by_id), (500, 2000, 2, by_id)]
        ws, wi, wl = O.topk(O.scores(q, stored), 7, 0.2, labels if by_id else None)
        assert np.array_equal(ix.numpy(), wi)
        np.testing.assert_allclose(sc.numpy(), ws, rtol=0, atol=1e-6)
        # row mode reports the label of each returned row
        assert np.array_equal(lb.numpy(), np.where(wi >= 0, labels[np.maximum(wi, 0)], -1) if not by_id else wl)


def test_npz_round_trip_across_dtypes(stub, tmp_path):
    rng = np.random.default_rng(5)
    g = gallery_mod.FaceGallery(40, dtype="bf16", device="cpu")
    g.enroll(torch.tensor(rng.standard_normal((50, 40)), dtype=torch.float32), np.arange(50) * 3)
    g.save(str(tmp_path / "g.npz"))
    z = np.load(str(tmp_path / "g.npz"))
    assert z["features"].dtype == np.float32 and z["features"].shape == (50, 40) and z["labels"].tolist() == list(range(0, 150, 3))
    h = gallery_mod.FaceGallery.load(str(tmp_path / "g.npz"), dtype="f32", device="cpu")
    assert len(h) == 50 and h.dtype == "f32" and h.labels.tolist() == list(range(0, 150, 3))
    # the bf16 rows come back as fp32 and are renormalised (|bf16(g)| differs from 1 by ~1e-4)
    assert torch.allclose(h.features(), g.features(), rtol=0, atol=2e-3)
    h.save(str(tmp_path / "h.npz"))
    b = gallery_mod.FaceGallery.load(str(tmp_path / "h.npz"), dtype="bf16", device="cpu")
    assert torch.allclose(b.features(), g.features(), rtol=0, atol=4e-3) and torch.equal(b.labels, g.labels)


def test_search_and_enroll_argument_checks(stub):
    g = gallery_mod.FaceGallery(8, dtype="f32", device="cpu")
    x = torch.zeros((2, 8))
    with pytest.raises(ValueError):
        g.enroll(torch.zeros((2, 7)), [0, 1])
    with pytest.raises(ValueError):
        g.enroll(x, [0])
    with pytest.raises(ValueError):
        g.enroll(x.double(), [0, 1])
    g.enroll(torch.ones((2, 8)), [4, 5])
    for bad in (0, 33, 2.0):
        with pytest.raises(ValueError):
            g.search(x, k=bad)
    with pytest.raises(ValueError):
        g.search(x, sim_th=float("nan"))
    with pytest.raises(ValueError):
        g.search(torch.zeros((2, 9)))
    with pytest.raises(ValueError):
        gallery_mod.FaceGallery(1025, device="cpu")
    with pytest.raises(ValueError):
        gallery_mod.FaceGallery(8, dtype="f16", device="cpu")
    empty = gallery_mod.FaceGallery(8, dtype="f32", device="cpu")
    sc, ix, lb = empty.search(x, k=3)
    assert ix.tolist() == [[-1] * 3] * 2 and lb.tolist() == [[-1] * 3] * 2 and bool(torch.isinf(sc).all())


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.efm_gallery_workspace_bytes(10, 2, 33) == 0 and lib.efm_gallery_workspace_bytes(10, 2, 0) == 0
    assert lib.efm_gallery_workspace_bytes(0, 1, 1) == 0 and lib.efm_gallery_workspace_bytes(10, 0, 1) == 0
    assert lib.efm_gallery_workspace_bytes(10, 3, 5) == 3 * lib.efm_gallery_workspace_bytes(10, 1, 5) > 0
    fake = ctypes.c_void_p(4096)   # never dereferenced: every check precedes the launch
    assert lib.efm_gallery_scan(fake, 4, 342, 342, fake, 1, 100, 352, None, 0, 33, 0.0, fake, 0, None) == -1
    assert b"k = 33 outside 1..32" in lib.efm_last_error_string()
    assert lib.efm_gallery_scan(fake, 4, 342, 342, fake, 1, 100, 342, None, 0, 5, 0.0, fake, 0, None) == -1
    assert b"ldg" in lib.efm_last_error_string()
    assert lib.efm_gallery_scan(fake, 4, 1100, 1100, fake, 1, 100, 1120, None, 0, 5, 0.0, fake, 0, None) == -1
    assert lib.efm_gallery_scan(fake, 4, 342, 342, fake, 1, 100, 352, None, 2 ** 31 - 50, 5, 0.0, fake, 0, None) == -1
    assert b"int32" in lib.efm_last_error_string()
    assert lib.efm_gallery_scan(fake, 4, 342, 342, fake, 1, 100, 352, None, 0, 5, float("nan"), fake, 0, None) == -1
    assert lib.efm_gallery_scan(None, 4, 342, 342, fake, 1, 100, 352, None, 0, 5, 0.0, fake, 0, None) == -1
    assert lib.efm_gallery_merge(fake, 1, 4, 40, 0, fake, fake, None, None) == -1
    assert b"gallery_merge" in lib.efm_last_error_string()
    assert lib.efm_gallery_pack(fake, 4, 342, 342, fake, 1, 350, None) == -1
    assert lib.efm_gallery_pack(fake, 4, 342, 300, fake, 1, 352, None) == -1


# --------------------------------------------------------------------------------------------- identify_efm.py metrics
def _write_csvs(d, name, feats, labels):
    with open(os.path.join(d, "feature_vector_%s.csv" % name), "w") as f:
        for r in feats:
            f.write("".join("{},".format(float(e)) for e in r) + "\n")
    with open(os.path.join(d, "label_%s.csv" % name), "w") as f:
        for v in labels:
            f.write("{}\n".format(float(v)))


def test_identify_metrics_on_hand_made_csvs(tmp_path):
    sys.path.insert(0, ROOT)
    import identify_efm as I
    e = np.eye(8, dtype=np.float32)
    # gallery: identities 0..5 at axes 0..5 (two rows each: the axis and a weaker copy)
    gf = np.concatenate([e[:6], 0.5 * e[:6] + 0.5 * e[6]])
    gl = np.concatenate([np.arange(6), np.arange(6)])
    # probes 0, 1: exact; probe 2 (identity 2) is nearer identity 3; probe 3 (identity 3) scores only 0.30; probes 4, 5 are identity 7,
    # which is not enrolled: 0.90 e0 + 0.44 e7 looks like identity 0 at 0.898, e7 scores 0 against everything
    pf = np.stack([e[0], e[1], 0.6 * e[2] + 0.8 * e[3], 0.3 * e[3] + 0.95 * e[7], 0.9 * e[0] + 0.44 * e[7], e[7]])
    pl = np.array([0, 1, 2, 3, 7, 7])
    _write_csvs(str(tmp_path), "train", gf, gl)
    _write_csvs(str(tmp_path), "valid", pf, pl)
    gf2, gl2 = I.read_features(str(tmp_path / "feature_vector_train.csv")), I.read_labels(str(tmp_path / "label_train.csv"))
    pf2, pl2 = I.read_features(str(tmp_path / "feature_vector_valid.csv")), I.read_labels(str(tmp_path / "label_valid.csv"))
    assert np.array_equal(gf2, gf) and gl2.tolist() == gl.tolist() and pf2.shape == (6, 8) and pl2.tolist() == pl.tolist()

    def search(k, th):
        sc, _, lb = O.topk(O.scores(pf2, gf2 / np.linalg.norm(gf2, axis=1, keepdims=True)), k, th, gl2)
        return sc, lb

    r = I.evaluate(gl2, pl2, search, [0.0, 0.5, 0.9])
    assert (r["known"], r["unknown"]) == (4, 2)
    assert r["rank1"] == 0.75 and r["rank5"] == 1.0
    # sim_th 0 accepts every probe (probe 2 with the wrong identity); 0.5 drops probe 3 and the e7 probe; 0.9 keeps the exact ones only
    assert r["open"] == [(0.0, 0.75, 1.0), (0.5, 0.5, 0.5), (0.9, 0.5, 0.0)]
    assert I.holdout_identities(pl2, 0.0).size == 0
    h = I.holdout_identities(np.arange(10), 0.2, seed=1)
    assert h.size == 2 and np.array_equal(h, I.holdout_identities(np.arange(10), 0.2, seed=1))
