"""CPU: the host side of the device augmentations (random_crop, color_jitter, random_erase): which names the transform
accepts, what draw_plan consumes from torch's generator and from python's `random` and what it decides -- against
tests/golden/augment_golden.npz (the reference's own Random2DTranslation / RandomErasing, Pillow's ImageEnhance) and, where
the reference tree is present, live against its classes -- and the numpy restatement of the pixel chain the GPU tests
compare the kernels with (tests/util_augment.py), byte for byte against the same goldens.  No GPU."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from ieee_amd.data import AugmentPlan, build_transforms
from ieee_amd.data import DeviceTransform as _DeviceTransform
from tests import util_augment as ua

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "augment_golden.npz"))
MEAN, STD = GOLD["mean"].tolist(), GOLD["std"].tolist()
DeviceTransform = functools.partial(_DeviceTransform, augment=True)     # (direct construction needs the opt-in)
ALL = ['random_flip', 'random_crop', 'color_jitter', 'random_erase']


class LoggingRandom(random.Random):
    """a random.Random that records (function, a, b, value) of every uniform / randint, as the golden generator recorded
    the reference's draws"""

    def __init__(self, seed):
        super().__init__(seed)
        self.rows = []

    def uniform(self, a, b):
        v = super().uniform(a, b)
        self.rows.append((0.0, float(a), float(b), float(v)))
        return v

    def randint(self, a, b):
        v = super().randint(a, b)
        self.rows.append((1.0, float(a), float(b), float(v)))
        return v


def test_the_reference_names_are_accepted_and_random_patch_is_not(capsys):
    tr = DeviceTransform(256, 128, ALL)
    assert _DeviceTransform.SUPPORTED == ('random_flip', 'random_crop', 'color_jitter', 'random_erase')
    assert tr.flip and tr.crop and tr.jitter and tr.erase and (tr.big_height, tr.big_width) == (288, 144)
    with pytest.raises(NotImplementedError, match="pool"):
        DeviceTransform(256, 128, ['random_flip', 'random_patch'])
    with pytest.raises(NotImplementedError):
        DeviceTransform(256, 128, ['random_rotate'])
    for name in ALL[1:]:        # constructed directly without the opt-in, the class takes the flip alone, as before
        with pytest.raises(NotImplementedError, match="augment=True"):
            _DeviceTransform(256, 128, [name])
    te = DeviceTransform(256, 128, ALL, train=False)
    assert not (te.flip or te.crop or te.jitter or te.erase or te.augments)
    with pytest.raises(ValueError):
        DeviceTransform(4, 4, ['random_crop'])
    capsys.readouterr()
    build_transforms(256, 128, ['random_erase', 'color_jitter', 'random_crop', 'random_flip'])
    lines = capsys.readouterr().out.splitlines()
    assert lines[:8] == ['Building train transforms ...', '+ resize to 256x128', '+ random flip',
                         '+ random crop (enlarge to 288x144 and crop 256x128)', '+ color jitter',
                         '+ to torch tensor of range [0, 1]',
                         '+ normalization (mean=%s, std=%s)' % (DeviceTransform(8, 8).mean.tolist(), DeviceTransform(8, 8).std.tolist()),
                         '+ random erase']
    assert lines[8] == 'Building test transforms ...' and len(lines) == 12
    build_transforms(256, 128, 'random_flip')
    assert not any('crop' in l or 'jitter' in l or 'erase' in l for l in capsys.readouterr().out.splitlines())


@pytest.mark.parametrize("tag,hw", [("ce", (64, 32)), ("ce_big", (256, 128))])
def test_crop_and_erase_draws_and_pixels_are_the_reference_classes(tag, hw):
    """the recorded run of the reference's Random2DTranslation -> ToTensor / Normalize -> RandomErasing: draw_plan makes the
    same calls with the same arguments and values in the same order, leaves `random` in the same state, and the plan pushed
    through the restatement gives the recorded tensors bit for bit"""
    tr = DeviceTransform(hw[0], hw[1], ['random_crop', 'random_erase'])
    imgs = GOLD[tag + "_in"]
    rng = LoggingRandom(int(GOLD[tag + "_seed"]))
    t0, p0 = torch.get_rng_state(), random.getstate()
    plan = tr.draw_plan(len(imgs), py_rng=rng)
    assert torch.equal(torch.get_rng_state(), t0) and random.getstate() == p0       # neither global generator was touched
    assert np.array_equal(np.asarray(rng.rows, dtype=np.float64), GOLD[tag + "_draws"])
    assert ua.digest(rng.getstate()) == str(GOLD[tag + "_state"])
    assert 0 < plan.crop[:, 0].sum() and (plan.erase[:, 2] > 0).any()
    if tag == "ce":
        assert plan.crop[:, 0].sum() < len(imgs) and (plan.erase[:, 2] == 0).any()   # both outcomes of both stages occur
    got = ua.apply_plan(list(imgs), plan, hw[0], hw[1], MEAN, STD, jitter=False)
    assert got.dtype == np.float32 and np.array_equal(got, GOLD[tag + "_out"])
    # the module-level generator is the default and is consumed identically
    random.seed(int(GOLD[tag + "_seed"]))
    assert tr.draw_plan(len(imgs)) == plan and ua.digest(random.getstate()) == str(GOLD[tag + "_state"])


def test_jitter_restatement_is_pillows_image_enhance():
    for k, first, b, c in GOLD["j_cases"]:
        got = ua.jitter_u8(GOLD["j_in"][int(k)], int(first), np.float32(b), np.float32(c))
        idx = int(np.flatnonzero((GOLD["j_cases"] == (k, first, b, c)).all(1))[0])
        assert np.array_equal(got, GOLD["j_out"][idx]), (k, first, b, c)
    assert np.array_equal(ua.jitter_u8(GOLD["j_big_in"], 1, np.float32(1.17), np.float32(0.88)), GOLD["j_big_out"])


def test_jitter_draw_order_and_generator_state():
    """the restated ColorJitter draw order (flip's rand(1), randperm(4), two uniform_) on the recorded seed"""
    rows = GOLD["jd_rows"]
    tr = DeviceTransform(64, 32, ['random_flip', 'color_jitter'])
    torch.manual_seed(int(GOLD["jd_seed"]))
    state = random.getstate()
    plan = tr.draw_plan(len(rows))
    assert random.getstate() == state                                      # flip and jitter never touch `random`
    assert ua.digest(torch.get_rng_state()) == str(GOLD["jd_state"])
    assert np.array_equal(plan.flip, rows[:, 0].astype(np.uint8))
    first = np.asarray([0 if list(r[1:5]).index(0) < list(r[1:5]).index(1) else 1 for r in rows], dtype=np.uint8)
    assert np.array_equal(plan.jitter_first, first) and set(first.tolist()) == {0, 1}
    assert np.array_equal(plan.jitter_b, rows[:, 5].astype(np.float32)) and np.array_equal(plan.jitter_c, rows[:, 6].astype(np.float32))
    assert plan.jitter_b.dtype == np.float32 and np.all((plan.jitter_b >= 0.8) & (plan.jitter_b <= 1.2))
    assert np.all((plan.jitter_c >= 0.85) & (plan.jitter_c <= 1.15))


@pytest.mark.parametrize("tag,hw", [("chain", (64, 32)), ("chain_big", (256, 128))])
def test_whole_chain_against_the_goldens(tag, hw):
    tr = DeviceTransform(hw[0], hw[1], ALL)
    n = int(GOLD[tag + "_n"])
    imgs = [GOLD["%s_in%d" % (tag, k)] for k in range(n)]
    random.seed(int(GOLD[tag + "_seed"]))
    torch.manual_seed(int(GOLD[tag + "_seed"]))
    plan = tr.draw_plan(n)
    assert ua.digest(random.getstate()) == str(GOLD[tag + "_py_state"])
    assert ua.digest(torch.get_rng_state()) == str(GOLD[tag + "_torch_state"])
    assert np.array_equal(ua.apply_plan(imgs, plan, hw[0], hw[1], MEAN, STD), GOLD[tag + "_out"])


def test_flip_only_plan_is_draw_flips_and_leaves_random_alone():
    tr = DeviceTransform(256, 128, 'random_flip')
    assert not tr.augments and not tr.needs_py_rng
    for n in (1, 5, 192):
        torch.manual_seed(31)
        flips = tr.draw_flips(n)
        after = torch.get_rng_state()
        torch.manual_seed(31)
        state = random.getstate()
        plan = tr.draw_plan(n)
        assert np.array_equal(plan.flip, flips) and torch.equal(torch.get_rng_state(), after) and random.getstate() == state
        assert not plan.crop.any() and not plan.erase.any() and np.all(plan.jitter_b == 1) and np.all(plan.jitter_c == 1)
    off = DeviceTransform(256, 128, ALL, train=False)
    t0 = torch.get_rng_state()
    assert not off.draw_plan(7).flip.any() and torch.equal(torch.get_rng_state(), t0) and random.getstate() == state


def test_erase_gives_up_after_100_attempts_and_draws_them_all():
    class Stubborn(LoggingRandom):
        def uniform(self, a, b):       # always erase; always the largest area at the smallest ratio: w = 52 >= W = 32
            v = 0.0 if (a, b) == (0, 1) else (b if b == 0.4 else a)
            self.rows.append((0.0, float(a), float(b), float(v)))
            return v
    tr = DeviceTransform(64, 32, ['random_erase'])
    rng = Stubborn(0)
    plan = tr.draw_plan(1, py_rng=rng)
    assert plan.erase[0].tolist() == [0, 0, 0, 0] and len(rng.rows) == 201      # the coin, 100 x (area, ratio), no randint


def test_plan_rows_of_a_global_batch_are_the_single_process_rows():
    tr = DeviceTransform(64, 32, ALL)
    G, mods, lo, hi = 16, 3, 4, 12
    random.seed(2); torch.manual_seed(2)
    whole = tr.draw_plan(G * mods)
    index = np.arange(G * mods).reshape(G, mods)
    random.seed(2); torch.manual_seed(2)
    again = tr.draw_plan(G * mods)                      # a rank seeded alike draws the same global plan ...
    for m in range(mods):
        shard = again[index[lo:hi, m]]                  # ... and keeps its rows of modality m
        assert len(shard) == hi - lo
        for j, i in enumerate(range(lo, hi)):
            assert shard[j] == whole[i * mods + m]
    assert whole[3:5] == whole[np.asarray([3, 4])] and len(whole[7]) == 1
    packed = whole.pack()
    assert packed.shape == (G * mods, 12) and packed.dtype == np.int32 and not packed[:, 11].any()
    assert np.array_equal(packed[:, 5].view(np.float32), whole.jitter_b) and np.array_equal(packed[:, 7:11], whole.erase)
    assert isinstance(whole[0:0], AugmentPlan) and len(whole[0:0]) == 0


def test_live_against_the_reference_classes():
    """a few hundred images through the reference's Random2DTranslation and RandomErasing themselves"""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    from PIL import Image
    ref_import.import_reference()
    from torchreid.data.transforms import Random2DTranslation, RandomErasing
    H, W, n = 32, 16, 300
    rs = np.random.RandomState(77)
    imgs = [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(n)]
    crop, erase = Random2DTranslation(H, W), RandomErasing(mean=MEAN)
    random.seed(99)
    want = []
    for im in imgs:
        u = np.asarray(crop(Image.fromarray(im, "RGB")))
        t = torch.from_numpy(u.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        t = t.sub_(torch.tensor(MEAN).view(3, 1, 1)).div_(torch.tensor(STD).view(3, 1, 1))
        want.append(erase(t).numpy())
    state = random.getstate()
    random.seed(99)
    tr = DeviceTransform(H, W, ['random_crop', 'random_erase'])
    plan = tr.draw_plan(n)
    assert random.getstate() == state
    assert 100 < plan.crop[:, 0].sum() < 200 and 100 < (plan.erase[:, 2] > 0).sum() < 200
    assert np.array_equal(ua.apply_plan(imgs, plan, H, W, MEAN, STD, jitter=False), np.stack(want))
