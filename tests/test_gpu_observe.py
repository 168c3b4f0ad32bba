"""bt_observe_window (batrack_amd/csrc/observe.hip) through batrack_amd.frontend.observe.window_observations against the
fixture tests/golden/observe_window.npz, which the reference's unmodified predict_target made: every output and every
touched buffer bit for bit, what the reference leaves alone unchanged, two calls identical bytes.  No tolerance."""
import numpy as np
import pytest
import torch

import observe_util as ou
from batrack_amd.frontend.observe import window_observations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return np.load(ou.GOLD)


def run(gold, case):
    args, kw, want = ou.load_case(gold, case, DEV)
    return ou.results(window_observations(*args, **kw), kw), want


@pytest.mark.parametrize("case", ou.CASES)
def test_op_equals_the_reference_bit_for_bit(gold, case):
    got, want = run(gold, case)
    for k in ou.OUTPUTS:
        assert ou.same_bits(got[k], want[k]), f"case {case}: {k} differs from the reference's"


@pytest.mark.parametrize("case", ou.CASES)
def test_op_leaves_alone_what_the_reference_leaves(gold, case):
    got, _ = run(gold, case)
    g = lambda k: gold[f"{case}.{k}"]
    n, Sp, kf = int(g("n")), int(g("Sp")), int(g("kf_stride"))
    rows = np.zeros(g("patches_valid_in").shape[0], bool)
    rows[n - Sp:n:kf] = True
    assert ou.same_bits(got["patches_valid"][~rows], g("patches_valid_in")[~rows])
    S_local = g("local_vis_in").shape[1]
    slot = g("jj") - g("ii") + (S_local + 1) // 2 - 1
    ok = (slot >= 0) & (slot < S_local)
    hit = np.zeros(g("local_vis_in").shape, bool)
    hit[g("kk")[ok], slot[ok]] = True
    for b in ou.BUFFERS:
        assert ou.same_bits(got[b][~hit], g(b + "_in")[~hit]), b


@pytest.mark.parametrize("case", ("a", "d_len", "e"))
def test_two_calls_give_identical_bytes(gold, case):
    a, _ = run(gold, case)
    b, _ = run(gold, case)
    for k in ou.OUTPUTS:
        assert ou.same_bits(a[k], b[k]), k


def test_inputs_are_not_written(gold):
    args, kw, _ = ou.load_case(gold, "d_len", DEV)
    before = [a.clone() for a in args]
    window_observations(*args, **kw)
    for a, b in zip(args, before):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_cpu_tensors_are_refused(gold):
    args, kw, _ = ou.load_case(gold, "a", "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        window_observations(*args, **kw)
