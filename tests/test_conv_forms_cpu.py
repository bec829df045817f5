"""Without a GPU: the table of tests/test_conv_forms_gpu.py selects, under ieee_conv_plan, the forms it names; the forms the table
covers close over every conv call net.hip makes on the layer grid of util_conv (22 ResNet-50 / CIM shapes + the padded stem, six
image sizes, twelve batch sizes, both types); the mask-from-statistics cases keep their kink share under the cap; and the float64
reference agrees with a nested-sum restatement."""
import json
import os
import subprocess
import sys

import pytest

from tests import util_bn as ub
from tests import util_conv as uc


@pytest.fixture(scope="module")
def lib():
    from ieee_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def child_plans(lib):
    """the child rows, planned in a child with the child's environment (the switch is read once per process)"""
    env = dict(os.environ, **uc.CHILD_ENV)
    r = subprocess.run([sys.executable, os.path.join(uc.ROOT, "tests", "util_conv.py"), "plan"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=uc.ROOT)
    return r


def test_every_row_selects_the_form_it_names(lib):
    bad = []
    for c in uc.cases(False):
        bad += uc.check_plan(lib, c)
    assert not bad, "\n".join(bad)
    names = [c.name for c in uc.cases(False)] + [c.name for c in uc.cases(True)]
    assert len(set(names)) == len(names)


def test_every_child_row_selects_the_wide_form(child_plans):
    r = child_plans
    assert r.returncode == 0 and "wide plans: 0 mismatches" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])
    assert all(c.want["BN"] in (64, 128) for c in uc.cases(True)) and any(c.want["BN"] == 128 for c in uc.cases(True))


def test_plan_query_needs_no_gpu_and_refuses_what_the_calls_refuse(lib):
    assert uc.plan(lib, "fwd", "f32", 3, 2, 16, 8, 64, 64, 3, 1, 1, uc.FL["sums"]) is None       # fused sums: bf16 vector path only
    assert uc.plan(lib, "fwd", "bf16", 3, 2, 16, 8, 3, 64, 7, 2, 3, uc.FL["sums"]) is None
    assert uc.plan(lib, "eval", "bf16", 3, 2, 16, 8, 3, 64, 7, 2, 3) is None
    assert uc.plan(lib, "dgrad", "bf16", 3, 2, 16, 8, 64, 64, 3, 1, 1, uc.FL["sums"] | uc.FL["bn2"]) is None   # patch form
    p = uc.plan(lib, "fwd", "bf16", 3, 2, 16, 8, 64, 64, 3, 1, 1)
    assert p["FAMILY"] == uc.PATCH and p["TILES_M"] == 2 and p["TILES_N"] == 1


def test_covered_forms_close_over_the_layer_grid(lib, child_plans):
    covered = {uc.form_key(c.op, c.dtype, uc.case_plan(lib, c)) for c in uc.cases(False)}
    line = [l for l in child_plans.stdout.splitlines() if l.startswith("KEYS ")]
    assert line, child_plans.stdout[-2000:]
    covered |= {tuple(k) for k in json.loads(line[0][5:])}
    missing = {}
    n = 0
    for (op, dtype, d, fl) in uc.grid_calls():
        p = uc.plan(lib, op, dtype, *d, flags=fl)
        n += 1
        if p is None:
            continue
        k = uc.form_key(op, dtype, p)
        if k not in covered:
            missing.setdefault(k, (op, dtype, d, fl))
    assert n > 10000
    assert not missing, "form keys no row covers (key: first call that selects it):\n" + "\n".join(
        "%s: %s" % kv for kv in sorted(missing.items(), key=str))


def test_mask_from_stats_cases_stay_off_the_kink():
    seen = 0
    for c in uc.cases(False) + uc.cases(True):
        if c.op == "dgrad" and c.sums and c.mask == "stats" and c.N * c.H * c.W * c.Ci * c.Co * c.R * c.R < 2e8:
            assert uc.kink_share(c) <= ub.KINK_CAP, c.name
            seen += 1
    assert seen >= 10


@pytest.mark.parametrize("stride,pad,R", [(1, 1, 3), (2, 1, 3), (2, 0, 1)])
def test_reference_agrees_with_nested_sums(stride, pad, R):
    key = ("f32", 2, 2, 5, 4, 3, 4, R, stride, pad)
    r = uc.Ref(key)
    for i in range(2):
        y, dx, dw = uc.nested(r.x[i], r.w[i], r.dy[i], stride, pad)
        for name, want in (("y", y.permute(0, 2, 3, 1)), ("dx", dx.permute(0, 2, 3, 1)), ("dw", dw)):
            got, A = r.get(name)
            assert float((got[i] - want).abs().max()) <= 1e-13 * float(A[i].max()), name
            assert bool((A[i] >= got[i].abs() - 1e-12).all())
