"""GPU: the ragged-batch resize (ieee_resize_normalize_ragged: N images of N sizes in one launch, Pillow's coefficients
computed on the device) is BIT-EXACT against the oracle chain, the Pillow goldens and the one-size kernel; its coefficient
function equals the host tables; DeviceTransform routes mixed lists through it; FeatureExtractor on top of it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util_ragged as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "transform_golden.npz"))
SENTINEL = -77.0
ERR_UNSUPPORTED = -3


def _transform(target):
    from ieee_amd.data import DeviceTransform
    return DeviceTransform(target[0], target[1], [], norm_mean=U.MEAN, norm_std=U.STD, train=False)


def _raw(images, flips, target, gap=0, mean=U.MEAN, std=U.STD):
    """one ieee_resize_normalize_ragged call as a C caller makes it: own packing (`gap` junk bytes before every image), dst
    between two sentinel images.  -> (status, dst [N + 2, 3, Ho, Wo] on the device, launches)"""
    from ieee_amd import _lib
    lib = _lib.require_gpu()
    n = len(images)
    offsets, at = [], 0
    for k, im in enumerate(images):
        at += gap + (k % 3 if gap else 0)
        offsets.append(at)
        at += im.size
    buf = np.full(at + gap, 0xAB, dtype=np.uint8)
    for im, off in zip(images, offsets):
        buf[off:off + im.size] = np.ascontiguousarray(im).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(n)
    sizes = np.asarray([im.shape[:2] for im in images], dtype=np.int32).reshape(n, 2)
    d_buf = torch.from_numpy(buf).cuda()
    d_off, d_sizes = torch.from_numpy(offsets).cuda(), torch.from_numpy(sizes).cuda()
    d_flip = None if flips is None else torch.from_numpy(np.asarray(flips, dtype=np.uint8)).cuda()
    dst = torch.full((n + 2, 3, target[0], target[1]), SENTINEL, dtype=torch.float32, device="cuda")
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    launches = ctypes.c_int(-1)
    status = lib.ieee_resize_normalize_ragged(
        _lib.ptr(d_buf), buf.size, _lib.ptr(d_off), _lib.ptr(d_sizes), _lib.ptr(d_flip), ctypes.c_void_p(offsets.ctypes.data),
        ctypes.c_void_p(sizes.ctypes.data), ctypes.c_void_p(dst[1:].data_ptr()), n, target[0], target[1], m, s,
        ctypes.byref(launches), _lib.stream())
    torch.cuda.synchronize()
    return status, dst, launches.value


@pytest.mark.parametrize("out_size", [256, 128, 64, 48, 7, 1])
def test_device_coefficients_equal_the_host_tables(out_size):
    """ksize, every bound and every weight of ieee_resample_coeffs == _axis_tables"""
    from ieee_amd import _lib
    from ieee_amd.data.transforms import _axis_tables
    lib = _lib.require_gpu()
    in_sizes = list(range(1, 521)) + [1023, 1024, 1025, 2047, 4095, 4096]
    tables = [_axis_tables(i, out_size) for i in in_sizes]
    total = sum(t[1].size for t in tables)
    bounds = torch.full((len(in_sizes), out_size, 2), -9, dtype=torch.int32, device="cuda")
    kk = torch.full((total,), -9, dtype=torch.int32, device="cuda")
    at = 0
    for j, (i, (_, k, ksize)) in enumerate(zip(in_sizes, tables)):
        assert lib.ieee_resample_ksize(i, out_size) == ksize, i
        _lib.check(lib.ieee_resample_coeffs(i, out_size, _lib.ptr(bounds[j]), ctypes.c_void_p(kk.data_ptr() + 4 * at), ksize,
                                            _lib.stream()))
        at += k.size
    bounds, kk = bounds.cpu().numpy(), kk.cpu().numpy()
    at = 0
    for j, (i, (b, k, ksize)) in enumerate(zip(in_sizes, tables)):
        assert np.array_equal(bounds[j], b), (i, out_size)
        assert np.array_equal(kk[at:at + k.size].reshape(k.shape), k), (i, out_size)
        at += k.size
    # a ksize that is not the axis's own (they are all odd) is refused
    spare = torch.zeros(2 * out_size, dtype=torch.int32, device="cuda")
    assert lib.ieee_resample_coeffs(5, out_size, _lib.ptr(spare), _lib.ptr(spare), 2, _lib.stream()) == -1
    assert lib.ieee_resample_ksize(4097, out_size) == 0


@pytest.mark.parametrize("target", U.TARGETS)
def test_one_ragged_call_is_bit_exact(target):
    """N = 37 over 18 sizes, alternating flips, custom mean / std, gaps between the images: every image equals the oracle
    chain; the sentinel images around dst are untouched; one launch"""
    sizes, flips = U.batch37()
    status, dst, launches = _raw([U.image(s) for s in sizes], flips, target, gap=5)
    assert status == 0 and launches == 1
    got = dst.cpu().numpy()
    assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL)
    for g, s, f in zip(got[1:-1], sizes, flips):
        assert np.array_equal(g, U.want(s, target, f)), (s, f)


@pytest.mark.parametrize("target", U.TARGETS)
def test_ragged_equals_the_one_size_kernel(target):
    """one behaviour, not two: tr.ragged == tr([img], flips=[f]) per image, for the sizes of the list and for the shapes on
    which the horizontal-first resampler and Pillow part ways"""
    tr = _transform(target)
    sizes = U.SIZES + U.DEVIATING
    images = [U.image(s) for s in sizes]
    flips = [(i + 1) % 2 for i in range(len(sizes))]
    got = tr.ragged(images, flips=flips)
    assert tr.last_ragged_launches == 1
    for i, s in enumerate(sizes):
        assert torch.equal(got[i], tr([images[i]], flips=[flips[i]])[0]), s


def test_goldens_in_one_call():
    from ieee_amd.data import DeviceTransform
    from oracle import transforms as ot
    tr = DeviceTransform(256, 128, "random_flip")
    n = len(GOLD["sizes"])
    flips = [int(bool(GOLD["flip%d" % i])) for i in range(n)]
    got = tr.ragged([GOLD["in%d" % i] for i in range(n)], flips=flips).cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], ot.to_tensor_normalize(GOLD["resized%d" % i], GOLD["mean"], GOLD["std"], bool(flips[i])))
        if "tensor%d" % i in GOLD.files:
            assert np.array_equal(got[i], GOLD["tensor%d" % i])


def test_one_image_no_image_no_flips_and_the_launch_count():
    target = (256, 128)
    size = (97, 33)
    status, dst, launches1 = _raw([U.image(size)], None, target)                     # N = 1, flip = NULL
    assert status == 0
    got = dst.cpu().numpy()
    assert np.array_equal(got[1], U.want(size, target, False)) and np.all(got[0] == SENTINEL) and np.all(got[2] == SENTINEL)
    sizes, flips = U.batch37()
    status, _, launches37 = _raw([U.image(s) for s in sizes], flips, target)
    assert status == 0 and launches1 == launches37 and 1 <= launches37 <= 3
    status, dst, launches0 = _raw([], None, target)                                   # N = 0: success, nothing launched
    assert status == 0 and launches0 == 0 and bool((dst == SENTINEL).all())
    tr = _transform(target)
    assert tr.ragged([]).shape == (0, 3, 256, 128)
    assert np.array_equal(tr.ragged([U.image(size)])[0].cpu().numpy(), U.want(size, target, False))


def test_a_side_of_4097_is_refused_before_any_launch():
    from ieee_amd import _lib
    target = (64, 48)
    for shape in ((4097, 2, 3), (2, 4097, 3)):
        images = [U.image((31, 96)), np.zeros(shape, dtype=np.uint8)]
        status, dst, launches = _raw(images, [0, 1], target)
        assert status == ERR_UNSUPPORTED and launches == 0
        assert b"4096" in _lib.load().ieee_last_error()
        assert bool((dst == SENTINEL).all())                     # not even the valid first image was written
    with pytest.raises(_lib.IeeeAmdError):
        _transform(target).ragged(images)


def test_an_image_outside_the_buffer_is_refused():
    from ieee_amd import _lib
    lib = _lib.require_gpu()
    im = U.image((31, 96))
    d_buf = torch.from_numpy(im.reshape(-1).copy()).cuda()
    offsets, sizes = np.asarray([16], dtype=np.int64), np.asarray([[31, 96]], dtype=np.int32)
    dst = torch.full((1, 3, 64, 48), SENTINEL, device="cuda")
    m = (ctypes.c_float * 3)(0, 0, 0)
    s = (ctypes.c_float * 3)(1, 1, 1)
    d_off, d_sizes = torch.from_numpy(offsets).cuda(), torch.from_numpy(sizes).cuda()
    status = lib.ieee_resize_normalize_ragged(
        _lib.ptr(d_buf), im.size, _lib.ptr(d_off), _lib.ptr(d_sizes), None,
        ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(sizes.ctypes.data), _lib.ptr(dst), 1, 64, 48, m, s, None,
        _lib.stream())
    torch.cuda.synchronize()
    assert status == -1 and bool((dst == SENTINEL).all())


def test_mixed_lists_are_routed_through_the_ragged_entry(monkeypatch):
    """DeviceTransform(256, 128, [])(mixed list): exactly one call of the new entry, none of the old one, the same bits"""
    from ieee_amd import _lib
    from ieee_amd.data import DeviceTransform
    lib = _lib.require_gpu()
    tr = DeviceTransform(256, 128, [])
    sizes = [(97, 33), (400, 40), (97, 33), (256, 128), (31, 96)]
    images = [U.image(s) for s in sizes]
    singles = [tr([im])[0].clone() for im in images]              # the one-size path, before the wrappers count
    calls = {"ragged": 0, "single": 0}
    old_ragged, old_single = lib.ieee_resize_normalize_ragged, lib.ieee_resize_flip_normalize

    def ragged(*a):
        calls["ragged"] += 1
        return old_ragged(*a)

    def single(*a):
        calls["single"] += 1
        return old_single(*a)
    monkeypatch.setattr(lib, "ieee_resize_normalize_ragged", ragged)
    monkeypatch.setattr(lib, "ieee_resize_flip_normalize", single)
    got = tr(images)
    assert calls == {"ragged": 1, "single": 0}
    for g, w, s in zip(got, singles, sizes):
        assert torch.equal(g, w), s
    tr([images[0], images[2]])                                    # one size in a list: the path it always took
    assert calls == {"ragged": 1, "single": 1}


@pytest.fixture(scope="module")
def extractor_case():
    from ieee_amd import FeatureExtractor
    from ieee_amd.models import build_model
    torch.manual_seed(11)
    model = build_model("ieee3modalPart", num_classes=1, pretrained=False, compute_dtype=torch.float32).cuda()
    fe = FeatureExtractor(model=model, image_size=(256, 128), batch_size=4, verbose=False)
    rng = np.random.RandomState(12)
    triples = [[rng.randint(0, 256, size=(int(rng.randint(40, 300)), int(rng.randint(20, 150)), 3)).astype(np.uint8)
                for _ in range(6)] for _ in range(3)]
    feats = fe(triples)
    return model, fe, triples, feats


def test_extractor_descriptors(extractor_case):
    model, fe, triples, feats = extractor_case
    tr = fe.preprocess
    assert feats.shape == (6, 2304) and feats.is_cuda and bool(torch.isfinite(feats).all())
    assert len(model._nets) == 1
    assert torch.equal(feats[:4], model([tr.ragged(r[:4]) for r in triples]))
    padded = model([tr.ragged(r[4:] + [r[5], r[5]]) for r in triples])
    assert torch.equal(feats[4:], padded[:2])
    assert len(model._nets) == 1


def test_extractor_reads_paths_like_arrays(extractor_case, tmp_path):
    from PIL import Image
    model, fe, triples, feats = extractor_case
    paths = []
    for m, row in enumerate(triples):
        paths.append([])
        for i, im in enumerate(row):
            paths[m].append(str(tmp_path / ("%d_%d.png" % (m, i))))
            Image.fromarray(im, "RGB").save(paths[m][-1])
    assert torch.equal(fe(paths), feats)
    assert torch.equal(fe([p[0] for p in paths]), fe([r[0] for r in triples]))       # a single path, a single array


def test_extractor_passes_float_tensors_through(extractor_case):
    model, fe, triples, feats = extractor_case
    tr = fe.preprocess
    tensors = [tr.ragged(r[:4]) for r in triples]
    seen = []
    hook = model.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    try:
        got = fe(tensors)
    finally:
        hook.remove()
    assert len(seen) == 1 and all(torch.equal(a, b) for a, b in zip(seen[0], tensors))
    assert torch.equal(got, feats[:4])
    assert torch.equal(fe([t[0] for t in tensors])[0], fe([t[:1] for t in tensors])[0])   # (3, H, W) is a batch of one
    assert len(model._nets) == 1


def test_extract_features_script():
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "scripts", "extract_features.py"),
                        "--synthetic", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "(5, 2304)", r.stdout[-2000:]


def test_a_worker_forked_from_another_thread_survives_a_ragged_call():
    """the loader starts its decode workers from the prefetch thread, by fork() where no fork server can be used.  A child
    forked from a thread destroys the thread-local objects of all other threads: the staging buffer (pinned) and its event
    must not be among them.  Fresh process: ragged calls on the main thread and on a second thread, then a fork from a
    third; the child must get as far as its own first statement."""
    code = ("import os, sys, threading; sys.path.insert(0, %r); import ieee_amd; import numpy as np; import torch\n"
            "from ieee_amd.data import DeviceTransform, pack_ragged\n"
            "tr = DeviceTransform(64, 48, [], train=False)\n"
            "imgs = [np.zeros((9, 7, 3), np.uint8), np.ones((5, 11, 3), np.uint8)]\n"
            "pack_ragged(imgs); tr(imgs); torch.cuda.synchronize()\n"
            "t = threading.Thread(target=lambda: DeviceTransform(64, 48, [], train=False)(imgs)); t.start(); t.join()\n"
            "torch.cuda.synchronize(); out = []\n"
            "def work():\n"
            "    pid = os.fork()\n"
            "    if pid == 0:\n"
            "        os._exit(0)\n"
            "    out.append(os.waitpid(pid, 0)[1])\n"
            "t = threading.Thread(target=work); t.start(); t.join(); print('child status', out[0])\n" % ROOT)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("child status 0"), (r.stdout[-500:], r.stderr[-1500:])
