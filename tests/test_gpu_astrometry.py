"""The offline plate solver (F21) on the GPU against tests/astrometry_model.py: the two kernels of csrc/astrometry.hip,
ops.solve_field, ApAstrometry and ap_astrometry end to end on a rendered frame, and the two new entry points under the memory guard.

What is held to what:
  sky_project  keep and the places of NaN equal the model's (its margins asserted first); xi and eta within 1e-12 degrees.  Each
               value is a quotient of products of three or four factors, each good to a few ulp of a magnitude <= 1, with at most one
               cancellation between terms of magnitude <= 1: under 1e-15 rad = 6e-14 degrees; 1e-12 degrees is 16 times that, and
               4e-8 px at 0.1 arcsec / px
  cell_select  idx, count, and inside where it is <= capacity, equal the model's exactly; two calls give the same bytes
  solve_field  the model's winning cell and pair set; CRVAL within 1e-9 degrees and CD within 1e-9 of its largest entry (the device's
               xi / eta differ by at most 1e-12 degrees and the centred fit is well conditioned: below 1e-10 expected); against the
               planted WCS the corner bound of the host test
Measured on an MI355X: see DESIGN 4.3m.
"""
import os

import numpy as np
import pytest

from astrophotography_amd import fitsio, wcs
from tests import astrometry_model as am
from tests import register_model as rm
from tests.test_astrometry_model_host import solved
from tests.test_gpu_register import _centroid_pairs, _render

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore::RuntimeWarning')]

torch = pytest.importorskip('torch')


def _ops():
    from astrophotography_amd import ops
    return ops


# ---- sky_project ------------------------------------------------------------------------------------------------------------------------
CENTRES = [(40.0, 0.0), (200.0, 62.0), (10.0, 89.9), (0.1, 20.0)]
COS_RC = float(np.cos(np.deg2rad(2.0)))


def _sky(n, centre, seed):
    """n stars: the first at the centre itself, most within 3 degrees of it (for ra0 = 0.1 many at ra about 359.9), and from 63 stars
    on some behind the tangent plane and rows with NaN / inf."""
    rng = np.random.default_rng(seed)
    ra0, dec0 = centre
    dec = np.clip(dec0 + rng.uniform(-3.0, 3.0, n), -90.0, 90.0)
    ra = np.mod(ra0 + rng.uniform(-3.0, 3.0, n) / max(np.cos(np.deg2rad(dec0)), 0.05), 360.0)
    ra[0], dec[0] = ra0, dec0
    if n >= 63:
        ra[5], dec[5] = ra0 + 180.0, -dec0                               # the antipode
        ra[6], dec[6] = ra0 + 170.0, 5.0 - dec0
        ra[7], dec[7] = ra0 + 90.0, 0.0                                  # on the horizon of the tangent point or near it
        ra[9], dec[10], ra[11], dec[12] = np.nan, np.nan, np.inf, -np.inf
        ra[13], dec[13] = np.nan, np.inf
        ra[20] = 359.9 if ra0 < 1.0 else ra[20]
    return ra, dec


@pytest.mark.parametrize('centre', CENTRES)
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_sky_project_against_the_model(n, centre):
    ra, dec = _sky(n, centre, 1000 * n + int(centre[1]))
    margin = rm.Margin()
    xi, eta, keep = am.project(ra, dec, centre[0], centre[1], COS_RC, margin)
    assert margin.value >= 1e-9
    gxi, geta, gkeep = (t.cpu().numpy() for t in _ops().sky_project(ra, dec, centre, COS_RC))
    assert gkeep.dtype == np.uint8 and np.array_equal(gkeep.astype(bool), keep)
    assert np.array_equal(np.isnan(gxi), np.isnan(xi)) and np.array_equal(np.isnan(geta), np.isnan(eta))
    assert not np.isinf(gxi).any() and not np.isinf(geta).any()
    ok = ~np.isnan(xi)
    near = ok & keep                                                     # the bound is derived for stars near the centre: the kept ones
    worst = max(float(np.abs(gxi[near] - xi[near]).max()), float(np.abs(geta[near] - eta[near]).max())) if near.any() else 0.0
    print('sky_project n = %d about %s: %d kept, %d behind the plane or not finite, largest difference %.3g deg' % (n, centre, keep.sum(), (~ok).sum(), worst))
    assert worst <= 1e-12
    assert gxi[0] == 0.0 and geta[0] == 0.0 and gkeep[0] == 1           # the star at the centre
    if n >= 63:
        assert not gkeep[[5, 6, 9, 10, 11, 12, 13]].any() and np.isnan(gxi[[5, 6, 9, 10, 11, 12, 13]]).all()
        far = ok & ~keep                                                 # in front of the plane, outside the cut: large tangents, relative bound
        assert np.all(np.abs(gxi[far] - xi[far]) <= 1e-12 * np.maximum(1.0, np.abs(xi[far]) ** 2))
        assert np.all(np.abs(geta[far] - eta[far]) <= 1e-12 * np.maximum(1.0, np.abs(eta[far]) ** 2))


def test_sky_project_empty_and_refusals():
    ops = _ops()
    xi, eta, keep = ops.sky_project(np.zeros(0), np.zeros(0), (10.0, 10.0), 0.5)
    assert xi.numel() == eta.numel() == keep.numel() == 0
    with pytest.raises(ValueError):
        ops.sky_project(np.zeros(3), np.zeros(4), (10.0, 10.0))
    from astrophotography_amd._lib import ApGpuError
    with pytest.raises(ApGpuError):
        ops.sky_project(np.zeros(3), np.zeros(3), (10.0, 95.0))


# ---- cell_select ------------------------------------------------------------------------------------------------------------------------
def _stars(n, seed):
    """n stars in [0, 1000)^2 with stars on the four inclusive edges of the cell (500, 500, 100), one 1 ulp outside it, and NaNs."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0.0, 1000.0, n), rng.uniform(0.0, 1000.0, n)
    special = [(600.0, 480.0), (400.0, 520.0), (470.0, 600.0), (530.0, 400.0), (np.nextafter(600.0, np.inf), 500.0), (500.0, np.nextafter(400.0, -np.inf)),
               (np.nan, 500.0), (500.0, np.nan), (np.nan, np.nan), (600.0, 600.0)]
    if n >= 63:
        at = rng.choice(n, size=len(special), replace=False)
        for i, (sx, sy) in zip(at, special):
            x[i], y[i] = sx, sy
    return x, y


CELLS3 = np.array([(500.0, 500.0, 100.0), (5000.0, 5000.0, 50.0), (500.0, 500.0, 1.0e4)])       # the edge cell, an empty one, one with all stars


def _check_cells(x, y, cells, capacity):
    idx, count, inside = am.cell_select(x, y, cells, capacity)
    g = _ops().cell_select(x, y, cells, capacity)
    gidx, gcount, ginside = (t.cpu().numpy() for t in g)
    assert gidx.dtype == gcount.dtype == ginside.dtype == np.int32 and gidx.shape == (len(cells), capacity)
    assert np.array_equal(gidx, idx) and np.array_equal(gcount, count)
    full = inside <= capacity
    assert np.array_equal(ginside[full], inside[full]) and np.all(ginside[~full] > capacity)
    return idx, count, inside, g


@pytest.mark.parametrize('capacity', [1, 7, 64, 512])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000, 5000])
def test_cell_select_equals_the_model(n, capacity):
    x, y = _stars(n, 7 * n + capacity)
    idx, count, inside, _ = _check_cells(x, y, CELLS3, capacity)
    finite = int((np.isfinite(x) & np.isfinite(y)).sum())
    assert inside[1] == 0 and count[1] == 0 and np.all(idx[1] == -1) and inside[2] == finite
    if n >= 63:
        xs, ys = x[idx[0][idx[0] >= 0]], y[idx[0][idx[0] >= 0]]
        if inside[0] <= capacity:                                        # the whole list: the four edge stars and the corner are in, the ulp outside is not
            assert (xs == 600.0).sum() == 2 and (xs == 400.0).sum() == 1 and (ys == 600.0).sum() == 2 and (ys == 400.0).sum() == 1
        assert not (xs > 600.0).any() and not (ys < 400.0).any()


@pytest.mark.parametrize('first,capacity', [(32, 64), (0, 7), (100, 512), (1000, 96)])
def test_cell_select_the_last_slot_falls_in_the_middle_of_a_wave(first, capacity):
    """All stars from index `first` on are inside: the capacity-th of them is at lane (first + capacity - 1) % 64, never 63."""
    n = 3000
    x = np.where(np.arange(n) < first, 2000.0, 500.0)
    y = np.full(n, 500.0)
    idx, count, inside, _ = _check_cells(x, y, [(500.0, 500.0, 10.0)], capacity)
    assert count[0] == capacity and idx[0, -1] == first + capacity - 1 and idx[0, -1] % 64 != 63


@pytest.mark.parametrize('C', [1, 3, 300])
def test_cell_select_many_cells_and_two_calls_give_the_same_bytes(C):
    x, y = _stars(5000, 11)
    rng = np.random.default_rng(C)
    cells = np.column_stack([rng.uniform(0, 1000, C), rng.uniform(0, 1000, C), rng.uniform(5, 300, C)])
    cells[0] = (500.0, 500.0, 100.0)
    _, _, _, a = _check_cells(x, y, cells, 64)
    b = _ops().cell_select(x, y, cells, 64)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    c = _ops().cell_select(xs, ys, torch.from_numpy(cells).cuda(), 64)
    for s, t in zip(a, c):
        assert torch.equal(s, t)


def test_cell_select_no_stars_no_cells_and_refusals():
    ops = _ops()
    idx, count, inside = ops.cell_select(np.zeros(0), np.zeros(0), CELLS3, 5)
    assert np.all(idx.cpu().numpy() == -1) and not count.any() and not inside.any()
    idx, count, inside = ops.cell_select(np.zeros(4), np.zeros(4), np.zeros((0, 3)), 5)
    assert tuple(idx.shape) == (0, 5) and count.numel() == 0
    nan_cell = ops.cell_select(np.full(9, 500.0), np.full(9, 500.0), [(np.nan, 500.0, 10.0), (500.0, 500.0, np.nan), (500.0, 500.0, 0.0)], 4)
    assert nan_cell[1].cpu().tolist() == [0, 0, 4] and nan_cell[2].cpu().numpy()[2] > 4
    for bad in (0, -1, 2 ** 20):
        with pytest.raises(ValueError):
            ops.cell_select(np.zeros(4), np.zeros(4), CELLS3, bad)
    with pytest.raises(ValueError):
        ops.cell_select(np.zeros(4), np.zeros(5), CELLS3, 4)


# ---- solve_field ------------------------------------------------------------------------------------------------------------------------
def _same_solution(got, want, what):
    assert got['status'] == want['status'] == am.NOMINAL, what
    assert got['cell'] == want['cell'] and got['parity'] == want['parity'] and got['n_seed'] == want['n_seed']
    assert np.array_equal(got['peak_votes'], want['peak_votes'])
    assert np.array_equal(got['pairs'], want['pairs']) and got['n_matched'] == want['n_matched']
    g, w = got['wcs'], want['wcs']
    d_crval = float(np.abs(g.crval - w.crval).max())
    d_cd = float(np.abs(g.cd - w.cd).max() / np.abs(w.cd).max())
    print('%s: CRVAL differs by %.3g deg, CD by %.3g of its largest entry, rms %.6f against %.6f px' % (what, d_crval, d_cd, got['rms'], want['rms']))
    assert np.array_equal(g.crpix, w.crpix)
    assert d_crval <= 1e-9 and d_cd <= 1e-9
    return d_crval, d_cd


@pytest.mark.parametrize('i', [0, 1])
def test_solve_field_against_the_model(i):
    f, want, margin = solved(i)
    assert margin >= 1e-9
    got = _ops().solve_field(f['xy'], f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'])
    _same_solution(got, want, 'field %d' % am.FIELDS[i][0])
    n = got['n_matched']
    corner = am.corner_error(got['wcs'], f['truth'], f['shape'])
    print('field %d: %d matched, corner error %.4f px (bound %.4f)' % (am.FIELDS[i][0], n, corner, 5.0 * am.SIGMA * np.sqrt(7.0 / n)))
    assert corner <= 5.0 * am.SIGMA * np.sqrt(7.0 / n)
    assert abs(got['cell_scale'] - want['cell_scale']) <= 1e-9 and abs(got['scale'] - want['scale']) <= 1e-9 * want['scale']


def test_solve_field_takes_tensors_and_drops_non_finite_rows():
    f, want, _ = solved(0)
    cat = {k: np.concatenate([[np.nan, 1.0, np.inf], v]) for k, v in f['cat'].items()}          # three rows with a non-finite value in front
    cat['dec'][1] = np.nan
    cat = {k: torch.from_numpy(v).cuda() for k, v in cat.items()}
    got = _ops().solve_field(torch.from_numpy(f['xy']), f['shape'], cat, f['centre'], f['s0'], 1.3, f['R'])
    assert got['status'] == am.NOMINAL and got['cell'] == want['cell']
    assert np.array_equal(got['pairs'][:, 0], want['pairs'][:, 0]) and np.array_equal(got['pairs'][:, 1], want['pairs'][:, 1] + 3)


def test_an_unrelated_list_has_no_solution_on_the_device():
    f = am.field(am.FIELDS[0])
    xy = am.unrelated_list(7, f['shape'])
    want, _ = am.solve_field(xy, f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'])
    got = _ops().solve_field(xy, f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'])
    assert want['status'] == am.NO_SOLUTION and got['status'] == _ops().SOLVE_NO_SOLUTION == am.NO_SOLUTION
    assert got['wcs'] is None and got['n_matched'] == 0 and not any(c['counted'] for c in got['candidates'])
    assert np.array_equal(got['peak_votes'], want['peak_votes'])


def test_use_sip_on_a_quadratic_distortion():
    """A planted quadratic distortion of 2 px at the corners: the SIP solution's matched rms is below the TAN solution's and its corner
    error within 5 sigma sqrt(13 / n) (12 parameters).  The model alone on 20 seeds stays within 0.93 of that bound."""
    ops = _ops()
    f = am.sip_field(1)
    args = (f['xy'], f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'])
    tan = ops.solve_field(*args)
    sip = ops.solve_field(*args, use_sip=True)
    want, margin = am.solve_field(*args, use_sip=True)
    assert margin >= 1e-9
    assert tan['status'] == sip['status'] == am.NOMINAL and isinstance(sip['wcs'], wcs.SipWcs) and isinstance(tan['wcs'], wcs.TanWcs)
    _same_solution(sip, want, 'SIP field')
    n = sip['n_matched']
    corner, corner_tan = (am.corner_error(s['wcs'], f['truth'], f['shape'], f['distort']) for s in (sip, tan))
    print('SIP: %d matched, rms %.4f px (TAN alone %.4f), corner error %.4f px (TAN alone %.4f; bound %.4f)'
          % (n, sip['rms'], tan['rms'], corner, corner_tan, 5.0 * am.SIGMA * np.sqrt(13.0 / n)))
    assert sip['rms'] < tan['rms']
    assert corner <= 5.0 * am.SIGMA * np.sqrt(13.0 / n)
    for k in ((2, 0), (1, 1), (0, 2)):
        assert abs(sip['wcs'].a.get(k, 0.0) - want['wcs'].a.get(k, 0.0)) <= 1e-12 and abs(sip['wcs'].b.get(k, 0.0) - want['wcs'].b.get(k, 0.0)) <= 1e-12


# ---- end to end on files ----------------------------------------------------------------------------------------------------------------
SIZE, SCALE = 512, 2.0


def _scene(seed, sky):
    """80 separated stars in a 512 x 512 frame under a planted WCS (2 arcsec / px, rotated, sky parity) and the catalogue they come
    from: those stars and 12000 more around the frame.  -> (image float32, truth WCS, true positions, catalogue dict)."""
    rng = np.random.default_rng(seed)
    pos = []
    while len(pos) < 80:                                                 # at least 14 px apart, 20 px inside the frame
        c = rng.uniform(20.0, SIZE - 21.0, size=2)
        if all((c[0] - q[0]) ** 2 + (c[1] - q[1]) ** 2 >= 14.0 ** 2 for q in pos):
            pos.append(c)
    pos = np.array(pos)
    ampl = 10.0 ** rng.uniform(np.log10(600.0), np.log10(30000.0), size=len(pos))
    truth = am.planted_wcs(sky, (SIZE, SIZE), SCALE, 25.0, False)
    ra, dec = truth.pix2sky(pos[:, 0], pos[:, 1])
    field = am.make_catalogue(seed + 1, sky, cone=2.2, n=12000)
    px, py = truth.sky2pix(field['ra'], field['dec'])
    out = ~((px > -5.0) & (px < SIZE + 4.0) & (py > -5.0) & (py < SIZE + 4.0))
    cat = dict(ra=np.concatenate([ra, field['ra'][out]]), dec=np.concatenate([dec, field['dec'][out]]),
               mag=np.concatenate([20.0 - 2.5 * np.log10(ampl), rng.uniform(8.8, 13.1, size=int(out.sum()))]))
    order = rng.permutation(len(cat['ra']))                              # a catalogue file is in no particular order
    return _render(pos, ampl, SIZE, rng), truth, pos, {k: v[order] for k, v in cat.items()}


def test_files_end_to_end(tmp_path):
    from astrophotography_amd.scripts import ap_astrometry, ap_find_stars
    sky = (150.25, -31.5)
    image, truth, pos, cat = _scene(2027, sky)
    img, src, out, catf, other = (str(tmp_path / n) for n in ('frame.fits', 'stars.fits', 'frame_wcs.fits', 'cat.fits', 'other.fits'))
    hdr = fitsio.Header()
    hint = am.unproject(0.08, -0.06, sky[0], sky[1])                     # the mount's idea of the centre: 0.1 degrees off
    hdr['RA-OBJ'], hdr['DEC-OBJ'] = hint
    hdr['XPIXSZ'], hdr['YPIXSZ'], hdr['FOCALLEN'] = 9.0, 9.0, 9.0e-3 / np.deg2rad(1.05 * SCALE / 3600.0)      # a plate scale 5 % off
    fitsio.write(img, image, hdr)
    fitsio.write_table(catf, [('CATALOG', {'RA_ICRS': cat['ra'], 'DE_ICRS': cat['dec'], 'Gmag': cat['mag'].astype(np.float32)}, None, None)])
    _, _, _, unrelated = _scene(4051, sky)
    fitsio.write_table(other, [('CATALOG', {'RA_ICRS': unrelated['ra'], 'DE_ICRS': unrelated['dec'], 'Gmag': unrelated['mag'].astype(np.float32)}, None, None)])
    assert ap_find_stars.main([img, src, '-q', '-l', 'ERROR']) == 0
    before = open(src, 'rb').read()
    flags = ['--ra_col', 'ra_icrs', '--dec_col', 'de_icrs', '--mag_col', 'gmag', '-l', 'ERROR']

    assert ap_astrometry.main([img, src, out, '--catalog', other] + flags) == 2        # the catalogue of another field
    assert not os.path.exists(out) and open(src, 'rb').read() == before

    assert ap_astrometry.main([img, src, out, '--catalog', catf] + flags) == 0
    data, h = fitsio.read(out)
    assert np.array_equal(data, image) and h['RA-OBJ'] == hint[0] and h['ASTCAT'] == 'cat.fits' and h['ASTPARIT'] == 1
    w = wcs.from_header(h)
    assert isinstance(w, wcs.TanWcs) and tuple(w.crpix) == (256.5, 256.5)
    cols, _, prim = fitsio.read_table(src, 'AP_L1MAG')
    found = np.stack([cols['xcenter'], cols['ycenter']], axis=1)
    e = _centroid_pairs(found, pos)
    assert len(e) >= 60
    sigma_c = float(np.sqrt(np.mean(e ** 2)))
    n = int(h['ASTNMAT'])
    corner = am.corner_error(w, truth, (SIZE, SIZE))
    print('sigma_c %.4f px; %d stars found, %d matched, rms %.4f px, scale %.5f, rotation %.3f deg, corner error %.4f px (bound %.4f)'
          % (sigma_c, len(found), n, h['ASTRMS'], h['ASTSCALE'], h['ASTROT'], corner, 5.0 * sigma_c * np.sqrt(7.0 / n)))
    assert n >= 50 and abs(h['ASTSCALE'] - SCALE) < 2e-3 and abs(h['ASTROT'] + 25.0) < 0.05       # planted_wcs turns the y axis 25 degrees west of north
    assert corner <= 5.0 * sigma_c * np.sqrt(7.0 / n)
    ra, dec = w.pix2sky(cols['xcenter'], cols['ycenter'])
    assert np.array_equal(cols['ra'], ra) and np.array_equal(cols['dec'], dec)
    assert prim['IMG_FILE'] == img and fitsio.read_table(src, 'AP_XYPOS')[0]['X'][0] == found[0, 0] + 1.0


# ---- the guard ------------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {'apgpu_sky_project', 'apgpu_cell_select'}


def _guard_case(io, shift):
    """Both new entry points with their inputs inside poisoned slabs, against the model."""
    ops = _ops()
    centre = (200.0, 62.0)

    def make():
        ra, dec = _sky(333, centre, 5)
        x, y = _stars(1500, 6)
        cells = np.concatenate([CELLS3, [(250.0, 750.0, 200.0), (900.0, 100.0, 150.0)]])
        return dict(ra=ra, dec=dec, x=x, y=y, cells=cells, proj=am.project(ra, dec, centre[0], centre[1], COS_RC),
                    sel={cap: am.cell_select(x, y, cells, cap) for cap in (7, 64)})
    d = io.once('data', make)
    xi, eta, keep = ops.sky_project(io.dev(d['ra'], shift), io.dev(d['dec'], shift), centre, COS_RC)
    kept = d['proj'][2]

    def near(got, ref, what):
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what
        assert np.all(np.abs(got[kept] - ref[kept]) <= 1e-12), what
    io.out('xi', xi, d['proj'][0], near)
    io.out('eta', eta, d['proj'][1], near)
    io.out('keep', keep, d['proj'][2].astype(np.uint8))
    x, y = io.dev(d['x'], shift), io.dev(d['y'], shift)
    for cap in (7, 64):
        idx, count, inside = ops.cell_select(x, y, d['cells'], cap)
        io.out('idx_%d' % cap, idx, d['sel'][cap][0])
        io.out('count_%d' % cap, count, d['sel'][cap][1])

        def inside_tol(got, ref, what, cap=cap):
            full = ref <= cap
            assert np.array_equal(got[full], ref[full]) and np.all(got[~full] > cap), what
        io.out('inside_%d' % cap, inside, d['sel'][cap][2], inside_tol)


@pytest.mark.parametrize('shift', [0, 1])
def test_new_entry_points_under_the_guard(shift, monkeypatch):
    """The protocol of tests/test_gpu_guard.py::test_guarded (runs A, B and C: poison 0xFF, poison 0x00, a side stream) for the two
    entry points this feature adds, through that module's runner - which also records them as covered for its own final count.  Both
    kernels are deterministic, so every result - `inside` of an overfull cell too - is compared between the runs bit for bit."""
    import test_gpu_guard as catalogue                                   # the module object pytest collected: its SEEN is the one counted
    fn = lambda io: _guard_case(io, shift)
    memo = {}
    default = torch.cuda.default_stream().cuda_stream
    assert torch.cuda.current_stream().cuda_stream == default
    A, sa = catalogue.run(fn, 0, 0xFF, memo, monkeypatch)
    assert {n for n, _ in sa} == NEW_ENTRY_POINTS
    assert all(s == default for _, s in sa)
    for label, got, ref, tol in A:
        catalogue.compare(got, ref, tol, '%s against the model' % label)
    B, _ = catalogue.run(fn, 0, 0x00, memo, monkeypatch)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = catalogue.run(fn, 0, 0xFF, memo, monkeypatch)
    assert [n for n, _ in sc] == [n for n, _ in sa] and all(s == side.cuda_stream for _, s in sc)
    for tag, other in (('B (poison 0x00)', B), ('C (side stream)', Cr)):
        assert [r[0] for r in other] == [r[0] for r in A]
        for (label, got, _, _), (_, first, _, _) in zip(other, A):
            catalogue.compare(got, first, 'bit', '%s, run %s against run A' % (label, tag))
    assert NEW_ENTRY_POINTS <= catalogue.SEEN
