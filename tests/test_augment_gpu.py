"""GPU: the device augmentations (ieee_augment_normalize: random crop, colour jitter, random erase behind the resize and the
flip) are BIT-EXACT against tests/golden/augment_golden.npz (the reference's own classes, Pillow's ImageEnhance) and against
the numpy restatement tests/util_augment.py (pinned to the same goldens by tests/test_augment_cpu.py): each stage alone and
all together, the stacked-tensor and the list path, forced edge plans, through the JPEG loader with and without prefetch, in
rank shards, within the launch budget, and into a training step.  Every comparison is array equality."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from tests import util_augment as ua

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "augment_golden.npz"))
MEAN, STD = GOLD["mean"].tolist(), GOLD["std"].tolist()
ALL = ['random_flip', 'random_crop', 'color_jitter', 'random_erase']


def _transform(h, w, names, **kw):
    from ieee_amd.data import DeviceTransform
    return DeviceTransform(h, w, names, augment=True, **kw)


def _both_paths(tr, imgs, plan):
    """the list path always; the stacked-tensor path too when the images have one size.  Returns the list path's result"""
    got = tr(list(imgs), plan=plan).cpu().numpy()
    if len({im.shape for im in imgs}) == 1:
        stacked = tr(torch.from_numpy(np.stack(imgs)), plan=plan).cpu().numpy()
        assert np.array_equal(stacked, got)
    return got


def _want(tr, imgs, plan):
    return ua.apply_plan(imgs, plan, tr.height, tr.width, tr.mean, tr.std, crop=tr.crop, jitter=tr.jitter, erase=tr.erase)


def _random_plan(tr, n, rs):
    """a plan with every enabled stage decided by `rs` (independent of the generators draw_plan consumes)"""
    from ieee_amd.data import AugmentPlan
    plan = AugmentPlan(n)
    H, W = tr.height, tr.width
    for i in range(n):
        plan.flip[i] = rs.randint(0, 2) if tr.flip else 0
        if tr.crop and rs.rand() < 0.6:
            plan.crop[i] = (1, rs.randint(0, tr.big_width - W + 1), rs.randint(0, tr.big_height - H + 1))
        if tr.jitter:
            plan.jitter_first[i] = rs.randint(0, 2)
            plan.jitter_b[i] = np.float32(rs.uniform(0.8, 1.2))
            plan.jitter_c[i] = np.float32(rs.uniform(0.85, 1.15))
        if tr.erase and rs.rand() < 0.6:
            h, w = rs.randint(1, H), rs.randint(1, W)
            plan.erase[i] = (rs.randint(0, H - h + 1), rs.randint(0, W - w + 1), h, w)
    return plan


def test_crop_and_erase_against_the_reference_classes_goldens():
    for tag, (H, W) in (("ce", (64, 32)), ("ce_big", (256, 128))):
        tr = _transform(H, W, ['random_crop', 'random_erase'])
        imgs = list(GOLD[tag + "_in"])
        plan = tr.draw_plan(len(imgs), py_rng=random.Random(int(GOLD[tag + "_seed"])))
        assert np.array_equal(_both_paths(tr, imgs, plan), GOLD[tag + "_out"]), tag
        # each of the two stages alone, from the same plan
        for names in (['random_crop'], ['random_erase']):
            one = _transform(H, W, names)
            assert np.array_equal(_both_paths(one, imgs, plan), _want(one, imgs, plan)), (tag, names)


def test_jitter_against_the_pillow_goldens():
    from ieee_amd.data import AugmentPlan
    tr = _transform(64, 32, ['color_jitter'])
    cases = GOLD["j_cases"]
    plan = AugmentPlan(len(cases))
    plan.jitter_first[:] = cases[:, 1].astype(np.uint8)
    plan.jitter_b[:] = cases[:, 2].astype(np.float32)
    plan.jitter_c[:] = cases[:, 3].astype(np.float32)
    imgs = [GOLD["j_in"][int(k)] for k in cases[:, 0]]
    got = _both_paths(tr, imgs, plan)
    from oracle.transforms import to_tensor_normalize
    for i in range(len(cases)):
        assert np.array_equal(got[i], to_tensor_normalize(GOLD["j_out"][i], MEAN, STD)), cases[i]
    big = _transform(256, 128, ['color_jitter'])
    plan = AugmentPlan(1)
    plan.jitter_first[0], plan.jitter_b[0], plan.jitter_c[0] = 1, np.float32(1.17), np.float32(0.88)
    assert np.array_equal(_both_paths(big, [GOLD["j_big_in"]], plan)[0], to_tensor_normalize(GOLD["j_big_out"], MEAN, STD))


def test_whole_chain_against_the_goldens():
    for tag, (H, W) in (("chain", (64, 32)), ("chain_big", (256, 128))):
        tr = _transform(H, W, ALL)
        imgs = [GOLD["%s_in%d" % (tag, k)] for k in range(int(GOLD[tag + "_n"]))]
        random.seed(int(GOLD[tag + "_seed"]))
        torch.manual_seed(int(GOLD[tag + "_seed"]))
        plan = tr.draw_plan(len(imgs))
        assert np.array_equal(_both_paths(tr, imgs, plan), GOLD[tag + "_out"]), tag      # ("chain": six source sizes in one list)
    # and drawn inside the call: the same seeds give the same tensor
    random.seed(int(GOLD["chain_big_seed"]))
    torch.manual_seed(int(GOLD["chain_big_seed"]))
    assert np.array_equal(tr([GOLD["chain_big_in0"]]).cpu().numpy(), GOLD["chain_big_out"])


@pytest.mark.parametrize("names", [['random_crop'], ['color_jitter'], ['random_erase'], ['random_flip', 'random_crop'],
                                   ['random_flip', 'color_jitter'], ['random_flip', 'random_erase'], ['random_crop', 'color_jitter'],
                                   ['color_jitter', 'random_erase'], ALL])
def test_random_sizes_and_random_plans_against_the_restatement(names):
    rs = np.random.RandomState(len(names) * 7 + len(names[0]))
    for (H, W), kw in (((64, 48), {}), ((128, 64), {}), ((50, 21), dict(norm_mean=[0.5, 0.4, 0.3], norm_std=[0.2, 0.25, 0.3]))):
        tr = _transform(H, W, names, **kw)                 # (50 x 21: 56.25 and 23.625 round to 56 x 24)
        sizes = [(H, W), (H + 1, W - 1), (31, 96), (200, 17), (H, 200), (130, W), (H, W), (2, 300), (H * 2, W * 2)]
        imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
        imgs.append(np.full((H, W, 3), 255, dtype=np.uint8))
        imgs.append((rs.randint(0, 8, size=(77, 40, 3)) + 100).astype(np.uint8))          # low contrast
        plan = _random_plan(tr, len(imgs), rs)
        assert np.array_equal(tr(imgs, plan=plan).cpu().numpy(), _want(tr, imgs, plan)), (H, W)
        same = [im for im in imgs if im.shape == (H, W, 3)]
        plan = _random_plan(tr, len(same), rs)
        assert np.array_equal(_both_paths(tr, same, plan), _want(tr, same, plan)), (H, W)


def test_forced_edge_plans():
    from ieee_amd.data import AugmentPlan
    rs = np.random.RandomState(3)
    for (H, W), kw in (((256, 128), {}), ((128, 64), {}), ((50, 21), dict(norm_mean=[0.1, 0.6, 0.9], norm_std=[0.5, 0.1, 0.3]))):
        tr = _transform(H, W, ALL, **kw)
        dx, dy = tr.big_width - W, tr.big_height - H
        crops = [(1, 0, 0), (1, dx, dy), (1, dx, 0), (1, 0, dy), (0, 0, 0), (1, dx // 2, dy // 2)]
        erases = [(0, 0, H - 1, W - 1), (1, 1, H - 1, W - 1), (0, 0, 1, W - 1), (H - 1, 0, 1, 1), (0, W - 1, H - 1, 1), (H - 3, W - 2, 3, 2),
                  (0, 0, 0, 0), (5, 0, 7, 3)]
        jitters = [(0, 0.8, 0.85), (0, 1.2, 1.15), (1, 0.8, 1.15), (1, 1.2, 0.85), (0, 0.8, 1.15), (1, 1.2, 1.15), (0, 1.0, 1.0), (1, 0.8, 0.85)]
        n = len(crops) * len(erases)
        plan = AugmentPlan(n)
        for i in range(n):
            plan.flip[i] = i % 2
            plan.crop[i] = crops[i % len(crops)]
            plan.erase[i] = erases[i // len(crops)]
            plan.jitter_first[i], plan.jitter_b[i], plan.jitter_c[i] = jitters[i % len(jitters)]
        imgs = [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(n)]
        imgs[1][:] = 255
        imgs[2][:] = 0
        imgs[3] = (imgs[3] // 64 + 250 - 3).astype(np.uint8)          # bright and flat: brightness 1.2 clips, contrast barely moves
        assert np.array_equal(_both_paths(tr, imgs, plan), _want(tr, imgs, plan)), (H, W)
        bad = plan[0:1]
        bad.crop[0] = (1, dx + 1, 0)
        with pytest.raises(ValueError):
            tr(imgs[:1], plan=bad)
        bad = plan[0:1]
        bad.erase[0] = (1, 0, H, 1)
        with pytest.raises(ValueError):
            tr(imgs[:1], plan=bad)
        with pytest.raises(ValueError):
            tr(imgs[:2], plan=plan[0:1])


def test_flip_only_and_eval_transforms_keep_their_path_and_bits():
    """'random_flip' alone (and train=False) do not go through the plan path: same entry point, same bits as before, and a
    plan handed to them contributes its flips only"""
    from ieee_amd.data import AugmentPlan
    from oracle.transforms import pil_bilinear_resize_u8, to_tensor_normalize
    rs = np.random.RandomState(4)
    imgs = [rs.randint(0, 256, size=(70, 30, 3)).astype(np.uint8) for _ in range(5)]
    tr = _transform(64, 32, 'random_flip')
    plan = AugmentPlan(5)
    plan.flip[:] = [1, 0, 1, 1, 0]
    plan.crop[:] = (1, 2, 3)
    plan.erase[:] = (0, 0, 9, 9)
    got = tr(torch.from_numpy(np.stack(imgs)), plan=plan).cpu().numpy()
    assert tr.last_launches is None                                   # ieee_augment_normalize was not called
    for i in range(5):
        assert np.array_equal(got[i], to_tensor_normalize(pil_bilinear_resize_u8(imgs[i], 64, 32), MEAN, STD, bool(plan.flip[i])))
    assert np.array_equal(tr(imgs, flips=plan.flip).cpu().numpy(), got)
    te = _transform(64, 32, ALL, train=False)
    assert np.array_equal(te(imgs).cpu().numpy()[1], got[1]) and te.last_launches is None


def test_launch_count_of_one_call_on_a_stacked_batch():
    """everything on: 5 launches with a horizontal resize pass (the limit is 6), whatever the batch size: no per-image launch;
    a stage that is off removes its launches"""
    rs = np.random.RandomState(5)
    for names, resized, same in ((ALL, 5, 4), (['random_flip', 'random_crop', 'random_erase'], 5, 4), (['random_flip', 'color_jitter'], 3, 2),
                                 (['random_flip', 'random_erase'], 2, 1), (['random_crop'], 5, 4)):
        tr = _transform(256, 128, names)
        for n in (1, 64):
            tr(torch.from_numpy(rs.randint(0, 256, size=(n, 300, 150, 3)).astype(np.uint8)))
            assert tr.last_launches == resized <= 6, (names, n)
            tr(torch.from_numpy(rs.randint(0, 256, size=(n, 256, 128, 3)).astype(np.uint8)))
            assert tr.last_launches == same, (names, n)


def _jpeg_tree(root, pids, per_id, size, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    names = ["%06d_cam%d_0_%02d.jpg" % (pid, 1 + k % 4, k) for pid in pids for k in range(per_id)]
    for split in ("train_171", "test"):
        for mod in ("RGB", "NI", "TI"):
            d = os.path.join(root, "RGBNT201", split, mod)
            os.makedirs(d)
            for nme in names:
                Image.fromarray(rng.randint(0, 256, size=size + (3,)).astype(np.uint8), "RGB").save(os.path.join(d, nme), quality=92)


def _record_plans(loader):
    seen = []
    orig = loader.transform.draw_plan

    def draw(n, py_rng=None):
        seen.append(orig(n, py_rng=py_rng))
        return seen[-1]
    loader.transform.draw_plan = draw
    return seen


def test_jpeg_loader_with_all_four_augmentations(tmp_path):
    """JPEG tree -> build_loaders(transforms = all four): every batch equals the restatement applied to the decoded files
    with the plans the loader drew (sample-major, modality-minor); prefetch = 0 and prefetch = 2 give the same batches bit for
    bit over three epochs (the sampler draws from `random` too: DeviceLoader._fork_plan_rng); two runs from the same seeds
    are identical"""
    from PIL import Image
    from ieee_amd import data as D
    _jpeg_tree(str(tmp_path), (3, 9, 20, 31), 4, (64, 32), 2)
    ds = D.RGBNT201(root=str(tmp_path))
    runs = []
    for prefetch in (0, 2, 2):
        random.seed(3); np.random.seed(3); torch.manual_seed(3)
        train, _, _ = D.build_loaders(ds, 96, 40, ALL, batch_size_train=8, workers=2, prefetch=prefetch)
        assert getattr(train, "_continuous", False) == (prefetch > 0)
        plans = _record_plans(train)
        out = []
        for epoch in range(3):
            n = 0
            for b in train:
                out.append((b['pid'].clone(), [x.clone() for x in b['img']], b['impath']))
                n += 1
            assert n == len(train)
        torch.cuda.synchronize()
        runs.append((out, plans))
        del train
    base, plans = runs[0]
    assert len(base) >= 6 and len(plans) == len(base)
    assert any(p.crop[:, 0].any() for p in plans) and any((p.erase[:, 2] > 0).any() for p in plans)
    for out, _ in runs[1:]:
        assert len(out) == len(base)
        for (p0, x0, _), (p1, x1, _) in zip(base, out):
            assert torch.equal(p0, p1) and all(torch.equal(a, b) for a, b in zip(x0, x1))
    for (pid, imgs, paths), plan in list(zip(base, plans))[:3]:
        index = np.arange(8 * 3).reshape(8, 3)
        for m in range(3):
            decoded = [np.asarray(Image.open(paths[i][m]).convert('RGB')) for i in range(8)]
            want = ua.apply_plan(decoded, plan[index[:, m]], 96, 40, D.transforms.IMAGENET_MEAN, D.transforms.IMAGENET_STD)
            assert np.array_equal(imgs[m].cpu().numpy(), want)


def test_two_rank_shards_together_are_the_single_process_batch(tmp_path):
    """two DeviceLoaders over ShardedIdentitySampler(.., rank, 2) in one process (no process group: every rank draws the
    order itself), seeded alike: the shards of global batch 0, in rank order, ARE the single-process loader's batch 0"""
    from ieee_amd import data as D
    from ieee_amd.data import sampler as smp
    from ieee_amd.data.loader import DeviceLoader
    _jpeg_tree(str(tmp_path), (3, 8, 11, 20), 2, (40, 24), 7)
    ds = D.RGBNT201(root=str(tmp_path))
    B, K, world = 8, 2, 2

    def seed():
        random.seed(4); np.random.seed(4); torch.manual_seed(9)
    seed()
    one = DeviceLoader(ds.train, _transform(64, 32, ALL), B, sampler=smp.build_train_sampler(ds.train, 'RandomIdentitySampler', batch_size=B,
                                                                                             num_instances=K), workers=0, drop_last=True)
    whole = next(iter(one))
    parts = []
    for r in range(world):
        seed()
        samp = smp.build_train_sampler(ds.train, 'RandomIdentitySampler', batch_size=B, num_instances=K, rank=r, world=world)
        loader = DeviceLoader(ds.train, _transform(64, 32, ALL), samp.local_batch, sampler=samp, workers=0, drop_last=True, global_rows=B)
        parts.append(next(iter(loader)))
        assert len(parts[-1]['pid']) == B // world and parts[-1]['global_rows'] == B
    assert torch.equal(torch.cat([p['pid'] for p in parts]), whole['pid'])
    for m in range(3):
        assert torch.equal(torch.cat([p['img'][m] for p in parts]), whole['img'][m])
    assert not torch.equal(parts[0]['img'][0], parts[1]['img'][0])


def test_engine_trains_on_cropped_and_erased_batches(tmp_path):
    """a few Image3MEngine steps on a synthetic tree with random_crop + random_erase on: the engine takes such batches and the
    loss stays finite"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import loader_probe
    from ieee_amd import data as D
    from ieee_amd.engine import Image3MEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    loader_probe.make_tree(str(tmp_path), n_ids=4, per_id=4, size=(128, 64))
    ds = D.RGBNT201(root=str(tmp_path))
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    train, _, _ = D.build_loaders(ds, 256, 128, ['random_flip', 'random_crop', 'random_erase'], batch_size_train=8, workers=2)

    class _DM(object):
        num_train_pids = ds.num_train_pids
        train_loader = train
        test_loader = {}
        sources = ["synthetic"]
    model = build_model("ieee3modalPart", num_classes=ds.num_train_pids, loss="margin", pretrained=False, use_gpu=True)
    eng = Image3MEngine(_DM(), model, build_optimizer(model, optim="sgd", lr=1e-3), margin=1, use_gpu=True)
    model.train()
    losses = []
    for epoch in range(2):
        for batch in train:
            assert batch['img'][0].shape == (8, 3, 256, 128)
            losses.append(float(eng.forward_backward(batch)["loss"]))
    assert len(losses) >= 3 and all(np.isfinite(l) for l in losses), losses
