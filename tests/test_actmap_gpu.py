"""GPU: activation maps on the device -- ieee_actmap_energy against the float64 restatement, ieee_actmap_render byte for
byte against the fp32 restatement (tests/util_actmap.py; why exact: tests/test_actmap_cpu.py), the model's
`return_featuremaps=True` / `trunk_maps` against the oracle's trunk, and visactmap end to end on an in-memory loader."""
import os

import numpy as np
import pytest
import torch

from tests import util_actmap as U
from tests.util_model import C, generated_state, images

pytestmark = pytest.mark.gpu

# Any fp32 summation order of n non-negative terms is within n * 2^-24 of the exact sum, relatively: 2048 * 2^-24 = 1.2e-4
# for the channel sum; the squares, the norm (a sum of at most 192 squares here, a square root) and the division add a
# few 2^-24 each.
ENERGY_RTOL = 2e-4


def _energy(x, out=None):
    from ieee_amd import _lib as L
    lib = L.require_gpu()
    N, P, Cc = x.shape
    out = torch.empty(N, P, dtype=torch.float32, device="cuda") if out is None else out
    dt = L.IEEE_BF16 if x.dtype == torch.bfloat16 else L.IEEE_F32
    status = lib.ieee_actmap_energy(L.ptr(x), dt, N, P, Cc, L.ptr(out), L.stream())
    return status, out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", U.ENERGY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_energy_matches_float64(shape, dtype):
    x = torch.from_numpy(U.energy_inputs(shape)).cuda().to(dtype)
    ref = U.energy_f64(x.float().cpu().numpy())          # the dtype-rounded values
    status, out = _energy(x)
    assert status == 0
    status, again = _energy(x)
    got = out.cpu().numpy()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("energy %s %s: max error %.3e of the largest value" % (shape, dtype, err))
    np.testing.assert_allclose(got, ref, rtol=ENERGY_RTOL, atol=0)
    np.testing.assert_allclose(np.sqrt((got.astype(np.float64) ** 2).sum(1)), 1.0, rtol=ENERGY_RTOL)
    assert status == 0 and torch.equal(out, again)      # fixed summation order: the same bits


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_energy_of_a_zero_image_is_zero(dtype):
    x = torch.from_numpy(U.energy_inputs((3, 128, 2048), seed=7)).cuda().to(dtype)
    status, alone = _energy(x)
    assert status == 0
    x[1].zero_()
    status, out = _energy(x, torch.full((3, 128), float("nan"), device="cuda"))
    assert status == 0
    assert torch.equal(out[1], torch.zeros(128, device="cuda"))             # zeros, not NaN
    assert torch.equal(out[0], alone[0]) and torch.equal(out[2], alone[2])    # the neighbours as without it
    assert float(out[0].abs().max()) > 0


def test_energy_rejects_bad_sizes():
    from ieee_amd import _lib as L
    x = torch.zeros(5000 * 16, dtype=torch.float32, device="cuda")
    out = torch.full((5000,), 7.0, device="cuda")
    for shape in ((1, 4, 12), (1, 5000, 8)):
        status = L.load().ieee_actmap_energy(L.ptr(x), L.IEEE_F32, shape[0], shape[1], shape[2], L.ptr(out), L.stream())
        assert status == -1, shape                                   # IEEE_ERR_BAD_ARG
        with pytest.raises(L.IeeeAmdError, match="actmap_energy"):
            L.check(status)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                  # nothing was launched


@pytest.mark.parametrize("name", [c[0] for c in U.RENDER_CASES])
def test_render_equals_the_fp32_restatement(name):
    from ieee_amd.reidtools import jet_table, render_actmaps
    amap, img, height, width = U.render_inputs(name)
    lut = jet_table()
    ref_grid, ref_index = U.render_f32(amap, img, U.IMAGENET_MEAN, U.IMAGENET_STD, lut, height, width)
    d_img = None if img is None else torch.from_numpy(img).cuda()
    grid, index = render_actmaps(d_img, torch.from_numpy(amap).cuda(), width, height, return_index=True)
    assert index.dtype == torch.uint8 and tuple(index.shape) == ref_index.shape
    bad = int((index.cpu().numpy() != ref_index).sum())
    print("%s: %d of %d indices differ" % (name, bad, ref_index.size))
    assert np.array_equal(index.cpu().numpy(), ref_index)
    if img is None:
        assert grid is None
        return
    assert grid.dtype == torch.uint8 and tuple(grid.shape) == ref_grid.shape
    g = grid.cpu().numpy()
    for panel, sl in (("image", slice(0, width)), ("gap 1", slice(width, width + 10)),
                      ("map", slice(width + 10, 2 * width + 10)), ("gap 2", slice(2 * width + 10, 2 * width + 20)),
                      ("overlay", slice(2 * width + 20, 3 * width + 20))):
        n_bad = int((g[:, :, sl] != ref_grid[:, :, sl]).sum())
        print("%s %s: %d bytes differ" % (name, panel, n_bad))
        assert n_bad == 0, panel
    assert np.array_equal(g, ref_grid)
    if "constant" in name:
        assert not index.any()                                       # a constant map: index 0 everywhere
    # a caller's own colour table is used as given; grids alone come back without return_index
    other = np.ascontiguousarray(lut[::-1])
    g2 = render_actmaps(d_img, torch.from_numpy(amap).cuda(), width, height, colormap=other)
    assert np.array_equal(g2.cpu().numpy()[:, :, width + 10:2 * width + 10], other[ref_index])


# ---- the model ---------------------------------------------------------------------------------------------------------
def _model(seed, dtype):
    from ieee_amd.models import build_model
    m = build_model("ieee3modalPart", num_classes=C, loss="margin", pretrained=False, use_gpu=True, compute_dtype=dtype)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = generated_state(shapes, seed)
    m.load_state_dict(sd)
    return m, sd


@pytest.fixture(scope="module")
def fp32_case():
    m, sd = _model(1, torch.float32)
    xs = images(4, 1)
    return m.eval(), sd, xs


def test_return_featuremaps_matches_the_oracle_trunk(fp32_case):
    from oracle import model as om
    m, sd, xs = fp32_case
    maps = m([x.cuda() for x in xs], return_featuremaps=True)
    assert isinstance(maps, list) and len(maps) == 3
    with torch.no_grad():
        for i in range(3):
            ref = om.resnet50_trunk(xs[i], sd, "backbone.%d." % i, False).numpy()
            got = maps[i]
            assert got.dtype == torch.float32 and tuple(got.shape) == (4, 2048, 16, 8) and got.is_contiguous()
            err, scale = np.abs(got.cpu().numpy() - ref).max(), np.abs(ref).max()
            print("modality %d: max |diff| %.3e at scale %.3e" % (i, err, scale))
            assert err <= 1e-3 + 1e-5 * scale                         # tests/test_model_gpu.py's rule
    # fresh tensors: another forward does not change them
    keep = maps[0].clone()
    m([x.cuda().flip(0) for x in xs])
    assert torch.equal(maps[0], keep)


def test_a_tensor_in_the_flag_position_is_not_a_request(fp32_case):
    m, sd, xs = fp32_case
    d = [x.cuda() for x in xs]
    fc = m(d, torch.zeros(4))                              # `timeids`, as the engine passes it
    assert torch.is_tensor(fc) and tuple(fc.shape) == (4, 2304)
    assert torch.equal(fc, m(d))
    assert tuple(m(d, torch.ones(1)).shape) == (4, 2304)   # truthy, but not True
    assert tuple(m(d, 1).shape) == (4, 2304)


def test_training_mode_refuses_feature_maps(fp32_case):
    m, sd, xs = fp32_case
    m.train()
    try:
        with pytest.raises(RuntimeError, match=r"call `model\.eval\(\)` first"):
            m([x.cuda() for x in xs], return_featuremaps=True)
        with pytest.raises(RuntimeError, match=r"call `model\.eval\(\)` first"):
            m.trunk_maps([x.cuda() for x in xs])
    finally:
        m.eval()


def test_nchw_list_and_native_view_give_the_same_maps(fp32_case):
    from ieee_amd.reidtools import activation_maps
    m, sd, xs = fp32_case
    d = [x.cuda() for x in xs]
    nchw = m(d, return_featuremaps=True)
    native = m.trunk_maps(d)
    assert native.dtype == torch.float32 and tuple(native.shape) == (3, 4, 16, 8, 2048)
    net = m.native_net(4, 256, 128)
    assert native.data_ptr() == net.tensor("backbone.{m}.layer4.2.conv3.a").data_ptr()      # a view: no copy
    a_native = activation_maps(native)
    a_list = activation_maps(nchw)
    assert a_native.dtype == torch.float32 and tuple(a_native.shape) == (3, 4, 16, 8)
    assert torch.equal(a_native, a_list)
    assert torch.equal(activation_maps(nchw[2]), a_native[2])
    ref = U.energy_f64(native.cpu().numpy().reshape(12, 128, 2048)).reshape(3, 4, 16, 8)
    np.testing.assert_allclose(a_native.cpu().numpy(), ref, rtol=ENERGY_RTOL, atol=0)


def test_bf16_trunk_maps_energy():
    """bf16 speed mode: the maps of the bf16 trunk output against the float64 energy of those same bf16 values (no claim
    across precisions: a random-init bf16 trunk is far from the fp32 one, tests/test_model_gpu.py)"""
    from ieee_amd.reidtools import activation_maps
    m, sd = _model(1, torch.bfloat16)
    m.eval()
    v = m.trunk_maps([x.cuda() for x in images(4, 1)])
    assert v.dtype == torch.bfloat16 and tuple(v.shape) == (3, 4, 16, 8, 2048)
    a = activation_maps(v)
    ref = U.energy_f64(v.float().cpu().numpy().reshape(12, 128, 2048)).reshape(3, 4, 16, 8)
    assert np.isfinite(ref).all() and ref.max() > 0
    np.testing.assert_allclose(a.cpu().numpy(), ref, rtol=ENERGY_RTOL, atol=0)


def test_visactmap_writes_the_figures(fp32_case, tmp_path, capsys):
    from PIL import Image
    from ieee_amd.reidtools import visactmap
    m, sd, xs = fp32_case
    height, width = 256, 128
    batches = []
    for b in range(2):
        imgs = [x[:3].clone() for x in images(4, 20 + b)]
        paths = [["/data/%s/%d_%d.jpg" % (mod, b, j) for j in range(3)] for mod in ("RGB", "NI", "TI")]
        batches.append({"img": imgs, "impath": paths})
    before = [[t.clone() for t in d["img"]] for d in batches]
    out = visactmap(m, {"synthetic": {"query": batches}}, str(tmp_path), "run", width, height, True, "TI")
    folder = os.path.join(str(tmp_path), "actmap_vis_run")
    names = ["%d_%d.jpg" % (b, j) for b in range(2) for j in range(3)]
    assert sorted(os.listdir(folder)) == names
    assert out == [os.path.join(folder, n) for n in names]
    for p in out:
        with Image.open(p) as im:
            assert im.size == (3 * width + 20, height) and im.mode == "RGB"
    for d, ref in zip(batches, before):
        for t, r in zip(d["img"], ref):
            assert t.device.type == "cpu" and torch.equal(t, r)      # the caller's tensors: where and what they were
    assert "Visualizing activation maps for synthetic ..." in capsys.readouterr().out
    # the figure on disk is the rendered one: its middle panel decodes close to the colour table's entries (JPEG, q 95)
    with Image.open(out[0]) as im:
        arr = np.asarray(im)
    assert (arr[:, width:width + 10] > 200).all()                     # the white gap
