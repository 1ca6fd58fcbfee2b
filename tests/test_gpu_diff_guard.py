"""The entry points of the optimal image subtraction (F23, csrc/subtract.hip) under the memory guard, by the protocol of
tests/test_gpu_guard.py (runs A, B and C: poison 0xFF, poison 0x00, a side stream; inputs unchanged afterwards), through that module's
runner, which records them as covered for its own final count.  The file carries this name, not that of tests/test_gpu_subtract.py
where the rest of the feature's GPU tests are, because that count is taken when tests/test_gpu_guard.py ends: the cases have to run
before it, and pytest runs the files in the order of their names."""
import numpy as np
import pytest

from tests import subtract_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

NEW_ENTRY_POINTS = {'apgpu_subtract_basis_f64', 'apgpu_subtract_stamps_f32', 'apgpu_subtract_apply_f32'}
LAUNCHING = NEW_ENTRY_POINTS - {'apgpu_subtract_basis_f64'}          # (the basis is host arithmetic: no stream argument)
H, W, HALF, RADIUS, KDEG, BDEG = 70, 90, 4, 5, 2, 1
SIGMAS, DEGREES = (0.8, 1.7), (2, 1)


def _guard_case(io, shift):
    from astrophotography_amd import ops

    def make():
        rng = np.random.default_rng(3)
        T = (100.0 + 40.0 * rng.random((H, W))).astype(np.float32)
        I = (50.0 + 0.8 * T + rng.standard_normal((H, W))).astype(np.float32)
        T[3, 4], I[60, 80], T[H - 1, W - 1] = np.nan, np.inf, np.nan
        mask = np.zeros((H, W), np.uint8)
        mask[40, 40] = 1
        F = HALF + RADIUS
        cen = np.array([(F, F), (W - 1 - F, H - 1 - F), (F - 1, 30), (40, 40), (60, 30), (30, 50), (70, 20), (20, 20), (50, 55), (75, 55)], np.int64)
        bs = sm.basis(SIGMAS, DEGREES, RADIUS)
        gram, status, count = sm.stamps(T, I, cen, HALF, bs, mask=mask, gain=1.5, readnoise=4.0)
        f = sm.fit(gram, status, count, cen, (H, W), KDEG, BDEG, rounds=0)
        kernels = sm.composites(f['akt'], bs)
        diff, matched = sm.apply(T, I, kernels, KDEG, f['bg'], BDEG)
        diff_i, _ = sm.apply(I, T, kernels, KDEG, f['bg'], BDEG, True, f['a0'])
        return dict(T=T, I=I, mask=mask, cen=cen, bs=bs, gram=gram, status=status, count=count, f=f, kernels=kernels, diff=diff, matched=matched,
                    diff_i=diff_i, sabs=sm.stamp_abs_sums(T, I, cen, HALF, bs, 1.5, 4.0))
    d = io.once('data', make)
    bs = ops.kernel_basis(SIGMAS, DEGREES, RADIUS)
    T, I, mask = io.dev(d['T'], shift), io.dev(d['I'], shift), io.dev(d['mask'], shift)
    gram, status, count = ops.subtract_stamps(T, I, d['cen'], HALF, bs, mask, 1.5, 4.0)

    def near(got, ref, what):
        ok = d['status'] == 0
        assert ok.sum() >= 5 and np.all(got[~ok] == 0.0), what
        assert np.all(np.abs(got[ok] - ref[ok]) <= (2 * HALF + 1) ** 2 * 2.0 ** -52 * d['sabs'][ok]), what
    io.out('gram', gram, d['gram'], near)
    io.out('status', status, d['status'])
    io.out('count', count, d['count'])
    diff, matched = ops.subtract_apply(T, I, d['kernels'], KDEG, d['f']['bg'], BDEG, matched=True)
    io.out('diff', diff, d['diff'])
    io.out('matched', matched, d['matched'])
    io.out('diff_image', ops.subtract_apply(I, T, d['kernels'], KDEG, d['f']['bg'], BDEG, True, d['f']['a0']), d['diff_i'])


@pytest.mark.parametrize('shift', [0, 1])
def test_new_entry_points_under_the_guard(shift, monkeypatch):
    """All kernels are deterministic, so every result is compared between the runs bit for bit."""
    import test_gpu_guard as catalogue                                   # the module object pytest collected: its SEEN is the one counted
    fn = lambda io: _guard_case(io, shift)
    memo = {}
    default = torch.cuda.default_stream().cuda_stream
    assert torch.cuda.current_stream().cuda_stream == default
    A, sa = catalogue.run(fn, 4 * W, 0xFF, memo, monkeypatch)
    assert {n for n, _ in sa} == LAUNCHING
    assert all(s == default for _, s in sa)
    for label, got, ref, tol in A:
        if ref is not None:
            catalogue.compare(got, ref, tol, '%s against the model' % label)
    B, _ = catalogue.run(fn, 4 * W, 0x00, memo, monkeypatch)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = catalogue.run(fn, 4 * W, 0xFF, memo, monkeypatch)
    assert [n for n, _ in sc] == [n for n, _ in sa] and all(s == side.cuda_stream for _, s in sc)
    for tag, other in (('B (poison 0x00)', B), ('C (side stream)', Cr)):
        assert [r[0] for r in other] == [r[0] for r in A]
        for (label, got, _, _), (_, first, _, _) in zip(other, A):
            catalogue.compare(got, first, 'bit', '%s, run %s against run A' % (label, tag))
    assert NEW_ENTRY_POINTS <= catalogue.SEEN
