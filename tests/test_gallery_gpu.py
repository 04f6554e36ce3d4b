"""The device-resident gallery on the GPU: the scan + merge kernels against the fp64 oracle of the selection rule
(tests/gallery_oracle.py), constructed edge cases, chunking, the end-to-end enrol / search of network features, identify_efm.py
and the C++ consumer of the C ABI."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from improving_face_recognition_performance_using_triplet_loss_amd.gallery import FaceGallery
from tests import gallery_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improving_face_recognition_performance_using_triplet_loss_amd")
TOL = 1e-5


def _unit(rng, m, d):
    x = rng.standard_normal((m, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _oracle_inputs(g, q):
    """The gallery rows as stored and the query as the kernel sees it (cast to the gallery dtype), both in fp64."""
    stored = g.features().double().cpu().numpy()
    qd = torch.as_tensor(q)
    if g.dtype == "bf16":
        qd = qd.to(torch.bfloat16)
    return stored, qd.double().numpy()


def _check(got, want, s_all, k):
    """Scores within TOL rank by rank; indices equal except for rare swaps among near-equal scores."""
    gs, gi, gl = (t.cpu().numpy() for t in got)
    ws, wi, wl = want
    assert gs.shape == ws.shape == (s_all.shape[0], k)
    assert np.array_equal(np.isinf(gs), np.isinf(ws)) and np.array_equal(gi < 0, wi < 0)
    fin = np.isfinite(ws)
    assert np.abs(gs[fin] - ws[fin]).max(initial=0.0) <= TOL
    diff = gi != wi
    for q, j in zip(*np.nonzero(diff)):
        # the kernel's row must score (in fp64) within the tolerance of the oracle's row at that rank
        assert abs(s_all[q, gi[q, j]] - ws[q, j]) <= 2 * TOL, (q, j, gi[q, j], wi[q, j])
    assert diff.sum() <= max(2, 0.01 * diff.size), "too many near-tie swaps: %d of %d" % (diff.sum(), diff.size)
    return gl


CASES = [  # (d, n, nq, k)
    (128, 1, 1, 1), (128, 17, 47, 5), (128, 4099, 1000, 32), (128, 300000, 47, 32),
    (342, 17, 1, 32), (342, 4099, 48, 5), (342, 300000, 1, 5), (342, 4099, 1000, 1),
    (684, 1, 48, 5), (684, 4099, 47, 32), (684, 300000, 48, 1), (684, 17, 1000, 32),
]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d,n,nq,k", CASES)
def test_search_matches_the_fp64_oracle(d, n, nq, k, dtype):
    rng = np.random.default_rng(d * 7 + n + nq * 3 + k)
    feats = _unit(rng, n, d)
    labels = rng.integers(0, max(n // 5, 1), size=n)
    q = _unit(rng, nq, d) * rng.uniform(0.5, 2.0, size=(nq, 1)).astype(np.float32)   # any query norm
    g = FaceGallery(d, dtype=dtype, device="cuda")
    g.enroll(torch.as_tensor(feats).cuda(), labels)
    stored, qd = _oracle_inputs(g, q)
    s_all = O.scores(qd, stored)
    sim_th = 0.05 if n >= 4099 else -1.0
    got = g.search(torch.as_tensor(q).cuda(), k=k, sim_th=sim_th)
    want = O.topk(s_all, k, sim_th)
    gl = _check(got, want, s_all, k)
    gi = got[1].cpu().numpy()
    assert np.array_equal(gl, np.where(gi >= 0, labels[np.maximum(gi, 0)], -1))
    got = g.search(torch.as_tensor(q).cuda(), k=k, sim_th=sim_th, by_identity=True)
    want = O.topk(s_all, k, sim_th, labels)
    gl = _check(got, want, s_all, k)
    gi = got[1].cpu().numpy()
    assert np.array_equal(gl, np.where(gi >= 0, labels[np.maximum(gi, 0)], -1))
    for row in gl:   # distinct identities
        ids = row[row >= 0]
        assert len(set(ids.tolist())) == ids.size


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_constructed_cases(dtype):
    d, n = 342, 5000
    rng = np.random.default_rng(11)
    feats = 0.02 * _unit(rng, n, d)
    q = _unit(rng, 3, d)
    feats[[7, 2500, 4999]] = q[0]                       # exact ties across tiles: resolved by row
    feats[[998, 999, 1000, 1001]] = q[1]                # ties straddling the boundary of 1000-row chunks
    feats[996] = q[1] + 0.5 * feats[996] / 0.02
    labels = np.arange(n) // 10
    for chunk_rows in (None, 1000):
        g = FaceGallery(d, dtype=dtype, device="cuda", chunk_rows=chunk_rows)
        g.enroll(torch.as_tensor(feats).cuda(), labels)
        qq = torch.as_tensor(np.concatenate([q, np.zeros((1, d), np.float32)])).cuda()
        s, i, lab = g.search(qq, k=4, sim_th=0.5)
        i = i.cpu().numpy()
        assert i[0].tolist() == [7, 2500, 4999, -1]
        assert i[1].tolist() == [998, 999, 1000, 1001]     # the 4th slot is the first row of the second chunk
        assert i[2].tolist() == [-1] * 4                   # everything below sim_th
        assert i[3].tolist() == [-1] * 4 and bool(torch.isinf(s[3]).all()) and lab[3].tolist() == [-1] * 4   # zero query
        s, i, _ = g.search(qq[1:2], k=5)
        assert i[0, :4].tolist() == [998, 999, 1000, 1001] and i[0, 4] == 996
        s, i, lab = g.search(qq[:2], k=3, sim_th=0.5, by_identity=True)
        assert lab.cpu().numpy().tolist() == [[0, 250, 499], [99, 100, -1]]   # rows 998, 999 -> identity 99; 1000, 1001 -> 100
        assert i.cpu().numpy().tolist() == [[7, 2500, 4999], [998, 1000, -1]]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_identity_owning_the_top_rows_does_not_hide_the_others(dtype):
    d, n = 128, 200
    rng = np.random.default_rng(5)
    q = _unit(rng, 1, d)[0].astype(np.float64)
    noise = rng.standard_normal((n, d))
    noise -= np.outer(noise @ q, q)                     # orthogonal to q
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    alpha = (0.99 - 0.004 * np.arange(n))[:, None]      # row i scores alpha_i: 0.004 apart, far above the bf16 rounding
    feats = (alpha * q + np.sqrt(1 - alpha ** 2) * noise).astype(np.float32)
    labels = np.concatenate([np.zeros(40, np.int64), 1 + (np.arange(n - 40) % 50)])
    g = FaceGallery(d, dtype=dtype, device="cuda")
    g.enroll(torch.as_tensor(feats).cuda(), labels)
    _, i, lab = g.search(torch.as_tensor(q[None].astype(np.float32)).cuda(), k=5, by_identity=True)
    assert lab[0].tolist() == [0, 1, 2, 3, 4] and i[0].tolist() == [0, 40, 41, 42, 43]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_three_chunks_equal_one(dtype):
    d, n = 342, 9000
    rng = np.random.default_rng(2)
    feats = _unit(rng, n, d)
    labels = rng.integers(0, 700, size=n)
    q = torch.as_tensor(_unit(rng, 60, d)).cuda()
    one = FaceGallery(d, dtype=dtype, device="cuda")
    many = FaceGallery(d, dtype=dtype, device="cuda", chunk_rows=3500)
    for gal in (one, many):
        gal.enroll(torch.as_tensor(feats[:4000]).cuda(), labels[:4000])
        gal.enroll(torch.as_tensor(feats[4000:]).cuda(), labels[4000:])
    assert len(many.chunks) == 3 and len(one.chunks) == 1
    for by_id in (False, True):
        a = one.search(q, k=32, sim_th=0.0, by_identity=by_id)
        b = many.search(q, k=32, sim_th=0.0, by_identity=by_id)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_enrolled_images_find_themselves():
    """Features of the EFM network on synthetic faces -> enrol -> search: every probe that is an enrolled image is its own rank-1
    match with score ~ 1."""
    from improving_face_recognition_performance_using_triplet_loss_amd import efm_symbol, synth
    from improving_face_recognition_performance_using_triplet_loss_amd.plan import Plan
    S, B = 128, 16
    data = efm_symbol.G.Variable("data")
    feat_sym, _ = efm_symbol.efm_feature(data)
    plan = Plan([feat_sym], (B, 1, S, S))
    flat = plan.new_flat()
    plan.init_xavier(flat, 3)
    feats = []
    for half in range(2):  # one synthetic identity per image
        faces = synth.identity_faces(torch.arange(half * B, (half + 1) * B), 1, S, 21 + half)
        (f,) = plan.forward(faces, flat, train=False)
        feats.append(f.view(B, -1)[:, :plan.outputs[0].shape[0]].double())
    feats = torch.cat(feats)
    assert feats.shape == (2 * B, 342)
    # an untrained network maps every face near one common direction: centre on the gallery mean (the LFW evaluator's `mean`)
    feats = (feats - feats.mean(0, keepdim=True)).float().contiguous()
    fn = torch.nn.functional.normalize(feats.double(), dim=1)
    cos = fn @ fn.T - 2 * torch.eye(2 * B, dtype=torch.float64, device=fn.device)
    closest = float(cos.max())
    assert closest < 0.99, "two synthetic faces have (almost) the same feature: cos %.5f" % closest
    labels = np.arange(2 * B) // 2
    for dtype in ("bf16", "f32"):
        g = FaceGallery(342, dtype=dtype, device="cuda")
        g.enroll(feats, labels)
        probes = feats[::3].contiguous()
        s, i, lab = g.search(probes, k=3)
        want = np.arange(0, 2 * B, 3)
        assert i[:, 0].cpu().numpy().tolist() == want.tolist()
        assert float((s[:, 0] - 1).abs().max()) < (1e-2 if dtype == "bf16" else 1e-5)
        assert lab[:, 0].cpu().numpy().tolist() == (want // 2).tolist()
        _, _, lab = g.search(probes, k=1, by_identity=True)
        assert lab[:, 0].cpu().numpy().tolist() == (want // 2).tolist()


def test_identify_script_runs_synthetic(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "identify_efm.py"), "--synthetic", "2000", "--sim-th", "0.3", "0.6"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"closed-set rank-1 ([\d.]+) rank-5 ([\d.]+)", r.stdout)
    assert m and 0.0 <= float(m.group(1)) <= float(m.group(2)) <= 1.0, r.stdout
    lines = re.findall(r"open-set sim_th ([\d.]+): accepted correctly ([\d.]+) \(enrolled\), accepted anyway ([\d.]+) \(not enrolled\)", r.stdout)
    assert [l[0] for l in lines] == ["0.300", "0.600"]
    assert float(lines[1][2]) <= float(lines[0][2]) and float(lines[1][1]) <= float(lines[0][1])


def test_cpp_gallery_consumer(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(os.path.join(PKG, "libefm_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "gallery_consumer")
    r = subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "gallery_consumer.cpp"),
                        "-L", PKG, "-lefm_hip", "-Wl,-rpath," + PKG, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gallery consumer: OK" in r.stdout
