"""F19 through its public interface (DESIGN 4.3e'): FITS files of one star field seen through planted lens distortion go through the
command lines - ap_register --model poly3, then ap_coadd and ap_drizzle with the transforms file it wrote - and through the classes
behind them (ApRegister.write_transforms, ApResample.coadd_files(maps=) with and without OVERSAMPLING, ApDrizzle.drizzle_files(maps=)
with rejection); and files with RA---TAN-SIP headers go through ap_coadd's WCS mode.  The stars of every result must sit where the truth
puts them: the per-axis rms of the centroid differences meets 3 sigma_c sqrt 2, the bound of
test_gpu_register.py::test_image_round_trip_512 (sigma_c: the star finder's own rms error on these frames), and the same files with
the distortion ignored do not.

Measured on an MI355X (profiles/f19_distortion/cli_round_trip.txt holds this module's output): see DESIGN 4.3e'.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_model as dm  # noqa: E402
import register_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = 512
SKY = 400.0


def _centroids(img, fwhm=3.0):
    import astrophotography_amd as ap
    t = ap.ApFindStars.from_device(img, search_fwhm=fwhm, loglevel='ERROR')._phot_table
    return np.stack([t['xcenter'], t['ycenter']], axis=1)


def _image(path):
    import torch
    from astrophotography_amd import fitsio
    data, hdr = fitsio.read(str(path))
    return torch.nan_to_num(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).cuda(), nan=SKY / 30.0), hdr


def _field(seed):
    rng = np.random.default_rng(seed)
    pos = []
    while len(pos) < 80:                                                 # at least 14 px apart, 20 px inside the frame
        c = rng.uniform(20.0, SIZE - 21.0, size=2)
        if all((c[0] - q[0]) ** 2 + (c[1] - q[1]) ** 2 >= 14.0 ** 2 for q in pos):
            pos.append(c)
    return np.array(pos), 10.0 ** rng.uniform(np.log10(600.0), np.log10(30000.0), size=80), rng


def _errors(found, truth):
    """(per-axis rms over all paired stars, the largest distance among the stars beyond 200 px from the centre, pairs)."""
    from tests.test_gpu_register import _centroid_pairs
    d = _centroid_pairs(found, truth)
    far = np.hypot(truth[:, 0] - 255.5, truth[:, 1] - 255.5) > 200.0
    dc = _centroid_pairs(found, truth[far])
    return float(np.sqrt(np.mean(d ** 2))), float(np.hypot(dc[:, 0], dc[:, 1]).max()), len(d), len(dc)


@pytest.fixture(scope='module')
def planted_files(tmp_path_factory):
    """Three 512 x 512 files, EXPOSURE 30 s: the reference and two frames under planted maps of 2 px at the corner (1.4 px cubic, 0.6
    px quadratic) with their own rotation and shift; frame 1 also holds 30 single-pixel hits.  -> (names, truth positions on the
    reference grid, sigma_c)."""
    import torch
    from astrophotography_amd import fitsio
    from tests.test_gpu_register import _centroid_pairs, _render
    pos, ampl, rng = _field(2028)
    maps = [None, dm.planted_map(SIZE, rot_deg=1.2, cubic_px=1.4, quad_px=0.6, shift=(5.4, -3.8)),
            dm.planted_map(SIZE, rot_deg=-0.7, cubic_px=1.4, quad_px=0.6, shift=(-2.25, 6.5))]
    d = tmp_path_factory.mktemp('distortion')
    names, err = [], []
    for k, f in enumerate(maps):
        p = pos if f is None else np.stack(f(pos[:, 0], pos[:, 1]), axis=1)
        img = _render(p, ampl, SIZE, rng)
        err.append(_centroid_pairs(_centroids(torch.from_numpy(img).cuda()), p))
        if k == 1:
            hit = rng.integers(30, SIZE - 30, size=(30, 2))
            img[hit[:, 1], hit[:, 0]] += 3000.0
        hdr = fitsio.Header()
        hdr['EXPOSURE'] = 30.0
        names.append(str(d / ('frame-%02d.fits' % k)))
        fitsio.write(names[-1], img, header=hdr)
    e = np.concatenate(err)
    assert len(e) >= 200
    return names, pos, float(np.sqrt(np.mean(e ** 2)))


def test_command_lines_put_the_corner_stars_where_the_truth_does(planted_files, tmp_path):
    yaml = pytest.importorskip('yaml')
    from astrophotography_amd.scripts import ap_coadd, ap_drizzle, ap_register
    names, pos, sigma_c = planted_files
    bound = 3.0 * sigma_c * np.sqrt(2.0)
    T = str(tmp_path / 'T.yml')
    assert ap_register.main(['-o', T, '--model', 'poly3', '-l', 'ERROR'] + names) == 0
    doc = yaml.safe_load(open(T))
    assert set(doc['transforms']) == set(doc['distortion']['frames']) == {os.path.basename(n) for n in names}
    assert [doc['distortion']['frames'][os.path.basename(n)]['order'] for n in names] == [1, 3, 3]
    assert [len(doc['distortion']['frames'][os.path.basename(n)]['x']) for n in names] == [3, 10, 10]
    assert doc['quality'][os.path.basename(names[1])]['order'] == 3
    # 2 px over 256 px is a hundred times the curvature of the 4096 x 4096 probe: its tiles cost 0.03 px, a quarter of the bound
    tile = ['--max_tile_error', '0.05', '-l', 'ERROR']
    out, flat = str(tmp_path / 'coadd.fits'), str(tmp_path / 'coadd_affine.fits')
    assert ap_coadd.main([out] + names + ['--transforms', T] + tile) == 0
    assert ap_coadd.main([flat] + names + ['--transforms', T, '--ignore_distortion', '-l', 'ERROR']) == 0
    img, hdr = _image(out)
    rms, corner, n, nc = _errors(_centroids(img), pos)
    rms_a, corner_a, na, _ = _errors(_centroids(_image(flat)[0]), pos)
    print('sigma_c %.4f px, bound %.4f px' % (sigma_c, bound))
    print('ap_coadd with the distortion entry: %d stars, per-axis rms %.4f px, corner stars (%d beyond 200 px) within %.4f px' % (n, rms, nc, corner))
    print('ap_coadd --ignore_distortion:       %d stars, per-axis rms %.4f px, corner stars within %.4f px' % (na, rms_a, corner_a))
    assert hdr['NCOMBINE'] == 3 and n >= 75 and nc >= 10
    assert rms <= bound
    assert rms_a > bound and corner_a > 3.0 * corner
    # the drizzle, with rejection: the output holds 2 pixels per reference pixel, pixel (u, v) at reference ((u + 0.5) / 2 - 0.5, ...)
    dz, wt = str(tmp_path / 'drizzle.fits'), str(tmp_path / 'drizzle_weight.fits')
    assert ap_drizzle.main([dz] + names + ['--transforms', T, '--scale', '2', '--pixfrac', '1.0', '--reject', '--weight_image', wt] + tile) == 0
    dimg, dhdr = _image(dz)
    assert tuple(dimg.shape) == (2 * SIZE, 2 * SIZE) and dhdr['COMBINET'] == 'DRIZZLE' and dhdr['DRIZNREJ'] >= 25
    found = (_centroids(dimg, fwhm=6.0) + 0.5) / 2.0 - 0.5
    rms_d, corner_d, nd, ncd = _errors(found, pos)
    print('ap_drizzle --scale 2 --reject:      %d stars, per-axis rms %.4f px, corner stars within %.4f px; %d pixels flagged'
          % (nd, rms_d, corner_d, dhdr['DRIZNREJ']))
    assert nd >= 75 and ncd >= 10
    assert rms_d <= bound
    assert (_image(wt)[0] > 0).float().mean().item() > 0.9


def test_classes_take_the_maps(planted_files, tmp_path):
    """The same files through the classes: ApRegister.maps() into ApResample.coadd_files(maps=) at OVERSAMPLING 2 (fine tiles from
    poly_tile_affines(tile_scale=n, scale=n)) and into ApDrizzle.drizzle(maps=) on tensors with and without rejection; a map too
    curved for its tiles is refused at the default max_tile_error."""
    import torch
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    names, pos, sigma_c = planted_files
    bound = 3.0 * sigma_c * np.sqrt(2.0)
    reg = ap.ApRegister('ERROR', model='poly3')
    reg.register_images(names)
    maps, affines = reg.maps(), reg.affines()
    assert [m.degree for m in maps] == [3, 3, 3] and reg.names() == [os.path.basename(n) for n in names]
    rs = ap.ApResample('ERROR', combine='MEDIAN', oversampling=2)
    out = str(tmp_path / 'coadd_os2.fits')
    with pytest.raises(ValueError, match='max_tile_error'):
        rs.coadd_files(names, affines, out, maps=maps)
    rs.coadd_files(names, affines, out, maps=maps, max_tile_error=0.05)
    rms, corner, n, nc = _errors(_centroids(_image(out)[0]), pos)
    print('ApResample(oversampling=2).coadd_files(maps=): %d stars, per-axis rms %.4f px (bound %.4f), corner stars within %.4f px' % (n, rms, bound, corner))
    assert n >= 75 and rms <= bound
    with pytest.raises(RuntimeError):
        rs.coadd_files(names, affines, out, maps=maps[:2], max_tile_error=0.05)
    frames = torch.stack([torch.from_numpy(np.ascontiguousarray(fitsio.read(n)[0], dtype=np.float32)).cuda() for n in names])
    plain = ap.ApDrizzle('ERROR', scale=2.0, pixfrac=1.0).drizzle(frames, affines, maps=maps, max_tile_error=0.05)
    rej = ap.ApDrizzle('ERROR', scale=2.0, pixfrac=1.0, reject=True).drizzle(frames, affines, maps=maps, max_tile_error=0.05)
    assert plain['rejected'] is None and rej['rejected'].tolist()[1] >= 25 and rej['rejected'].sum() < 400
    hot = (plain['image'] - rej['image']).abs() > 50.0                   # the hits are in the plain result and gone from the other
    assert 25 <= int(hot.sum()) <= 400
    for tag, r in (('plain', plain), ('reject', rej)):
        found = (_centroids(torch.nan_to_num(r['image'], nan=SKY), fwhm=6.0) + 0.5) / 2.0 - 0.5
        rms_d, corner_d, nd, _ = _errors(found, pos)
        print('ApDrizzle.drizzle(maps=), %s: %d stars, per-axis rms %.4f px, corner stars within %.4f px' % (tag, nd, rms_d, corner_d))
        assert nd >= 75 and rms_d <= bound
    with pytest.raises(ValueError):
        ap.ApDrizzle('ERROR').drizzle(frames, affines, maps=maps[:2], max_tile_error=0.05)


def test_ap_coadd_follows_sip_headers(tmp_path):
    """Three files with RA---TAN-SIP headers (orders 2, 3 and 2; 3 px at 250 px from CRPIX) and no transforms file: ap_coadd registers
    them through the sky where it refused them before, the output grid is the first file's pure TAN part, its header carries no SIP
    card, and the stars sit where that grid puts them."""
    import torch
    from astrophotography_amd import fitsio, wcs
    from astrophotography_amd.scripts import ap_coadd
    from tests.test_gpu_register import _centroid_pairs, _render
    pos, ampl, rng = _field(2029)
    s = 1.8 / 3600.0
    base = dict(CTYPE1='RA---TAN-SIP', CTYPE2='DEC--TAN-SIP', CRVAL1=303.0272359, CRVAL2=38.3549333)
    r2, r3 = 3.0 / 250.0 ** 2, 3.0 / 250.0 ** 3
    cards = [dict(base, CRPIX1=256.0, CRPIX2=257.0, CD1_1=-s, CD1_2=0.0, CD2_1=0.0, CD2_2=s, A_ORDER=2, B_ORDER=2, A_2_0=r2, A_0_2=0.5 * r2,
                  B_1_1=-r2, B_0_2=0.3 * r2),
             dict(base, CRPIX1=250.5, CRPIX2=262.25, CD1_1=-s * np.cos(0.02), CD1_2=s * np.sin(0.02), CD2_1=s * np.sin(0.02), CD2_2=s * np.cos(0.02),
                  A_ORDER=3, B_ORDER=3, A_2_0=-0.5 * r2, A_3_0=r3, A_1_2=r3, B_0_2=0.4 * r2, B_2_1=r3, B_0_3=r3),
             dict(base, CRPIX1=261.0, CRPIX2=251.5, CD1_1=-s, CD1_2=0.0, CD2_1=0.0, CD2_2=s, A_ORDER=2, B_ORDER=2, A_1_1=r2, B_2_0=-0.7 * r2)]
    out_wcs = wcs.from_header(cards[0]).tan()
    names, err, moved = [], [], 0.0
    for k, c in enumerate(cards):
        w = wcs.from_header(c)
        assert isinstance(w, wcs.SipWcs)
        p = np.stack(w.sky2pix(*out_wcs.pix2sky(pos[:, 0], pos[:, 1])), axis=1)
        moved = max(moved, float(np.hypot(*(p - np.stack(w.tan().sky2pix(*out_wcs.pix2sky(pos[:, 0], pos[:, 1])), axis=1)).T).max()))
        img = _render(p, ampl, SIZE, rng)
        err.append(_centroid_pairs(_centroids(torch.from_numpy(img).cuda()), p))
        hdr = fitsio.Header()
        hdr['EXPOSURE'] = 30.0
        for key, v in c.items():
            hdr[key] = v
        names.append(str(tmp_path / ('sip-%02d.fits' % k)))
        fitsio.write(names[-1], img, header=hdr)
    sigma_c = float(np.sqrt(np.mean(np.concatenate(err) ** 2)))
    bound = 3.0 * sigma_c * np.sqrt(2.0)
    assert moved > 2.0                                                   # the SIP terms move stars by pixels: ignoring them could not pass
    out = str(tmp_path / 'coadd_sip.fits')
    assert ap_coadd.main([out] + names + ['-l', 'ERROR']) == 0
    img, hdr = _image(out)
    assert str(hdr['CTYPE1']).strip() == 'RA---TAN' and str(hdr['CTYPE2']).strip() == 'DEC--TAN'
    assert not [k for k in hdr.keys() if wcs.is_sip_card(k)] and hdr['CRPIX1'] == 256.0 and hdr['NCOMBINE'] == 3
    rms, corner, n, nc = _errors(_centroids(img), pos)
    print('ap_coadd on three RA---TAN-SIP files (SIP terms move the stars by up to %.2f px): sigma_c %.4f px, bound %.4f px; %d stars, per-axis '
          'rms %.4f px, corner stars within %.4f px' % (moved, sigma_c, bound, n, rms, corner))
    assert n >= 75 and rms <= bound
