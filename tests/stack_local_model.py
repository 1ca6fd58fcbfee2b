"""The NumPy restatement of APGPU_STACK_FRAME_LOCAL (include/apgpu.h, csrc/stack_reject.hip): scale and offset of a frame as
meshes - one value per box_height x box_width box, the geometry of apgpu_box_clipped_stats_f32 - interpolated bilinearly at
every pixel inside the two rejection rules of small stacks.

Box centres lie at (j + 0.5) box - 0.5.  Per axis, with c the pixel coordinate, b the box size and m the mesh extent:

    u  = 2c + 1 - b                                         # whole numbers: exact
    j0 = clamp(floor(u / 2b), 0, max(m - 2, 0));  j1 = min(j0 + 1, m - 1)
    t  = float32(clamp(u - 2 b j0, 0, 2b)) / float32(2b)    # the one rounding

For a mesh M of frame i, every operation a float32 NumPy operation of its own:

    top = M[j0][k0] + tx * (M[j0][k1] - M[j0][k0]);  bot = the same on row j1;  m(y, x) = top + ty * (bot - top)

v = float32(float32(a(y, x) * x_raw) + b(y, x)); without a scale mesh v = float32(x_raw + b).  From there on everything is
tests/stack_frame_model.py: the rule on the finite v in frame order, count and std_f64 unweighted, mean_f64 the sequential
weighted sum over the survivors.
"""
import numpy as np

from tests import stack_frame_model as frame

F = np.float32


def axis_weights(n, b, m, c0=0):
    """The coordinates c0 .. c0 + n - 1 of an axis with boxes of b pixels and m mesh cells -> (j0, j1 int64 [n], t float32 [n])."""
    c = np.arange(c0, c0 + n, dtype=np.int64)
    u = 2 * c + 1 - b
    j0 = np.clip(np.floor_divide(u, 2 * b), 0, max(m - 2, 0))
    j1 = np.minimum(j0 + 1, m - 1)
    t = np.clip(u - 2 * b * j0, 0, 2 * b).astype(F) / F(2 * b)
    return j0, j1, t


def local_map(mesh, shape, box, row0=0):
    """A mesh [..., ny, nx] evaluated at the pixels of an image stripe of `shape` = (rows, W) that starts at image row row0:
    float32 [..., rows, W]."""
    mesh = np.asarray(mesh, F)
    bh, bw = (box, box) if np.ndim(box) == 0 else box
    ny, nx = mesh.shape[-2:]
    j0, j1, ty = axis_weights(shape[0], bh, ny, row0)
    k0, k1, tx = axis_weights(shape[1], bw, nx)
    ty = ty[:, None]
    r0, r1 = mesh[..., j0, :], mesh[..., j1, :]
    top = r0[..., k0] + tx * (r0[..., k1] - r0[..., k0])
    bot = r1[..., k0] + tx * (r1[..., k1] - r1[..., k0])
    return top + ty * (bot - top)


def local_values(cube, A, B, box, row0=0):
    """v of every pixel: float32 [N, rows, W].  A None: v = x + b."""
    x = np.asarray(cube).astype(F)
    with np.errstate(over='ignore', invalid='ignore'):
        if A is not None:
            x = local_map(A, x.shape[1:], box, row0) * x
        return x + local_map(B, x.shape[1:], box, row0)


def local_params(cube, A, B, w, box, method, row0=0, pixmask=None, **rule):
    """-> dict(mean_f64, std_f64, count, keep [N, rows, W] bool, v).  cube [N, rows, W]; A [N, ny, nx] or None; B [N, ny, nx];
    w [N] or None (ones); method 'winsorized' (kl, kh, maxiters) or 'minmax' (nlow, nhigh)."""
    v = local_values(cube, A, B, box, row0)
    N = v.shape[0]
    ones = np.ones(N, F)
    # the mapped values through the frame model with the identity map (1 * v + 0 = v, every bit and the sign of zero kept)
    r = frame.frame_params(v, ones, np.full(N, -0.0, F), ones if w is None else w, method, pixmask=pixmask, **rule)
    assert np.array_equal(r['v'].view(np.uint32)[np.isfinite(v)], v.view(np.uint32)[np.isfinite(v)])
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# the scene the local map was added for: a sky whose SHAPE differs from frame to frame
SCENE_SHAPE, SCENE_NOISE, TRAIL_ROW, TRAIL_FRAMES, TRAIL_ADU, SKY, AMPLITUDE = (96, 128), 8.0, 40, (2, 5), 120.0, 200.0, 150.0


def gradient_scene(N, seed=7):
    """The star field on 96 x 128 pixels, noise sigma 8; frame 0 flat at 200 ADU, frame i with the planar gradient
    200 + 150 (i / (N - 1)) 2 (cos th (x / (W - 1) - 0.5) + sin th (y / (H - 1) - 0.5)), th = 2 pi i / N; a +120 ADU trail on row 40
    of frames 2 and 5.  -> (cube float32 [N, 96, 128], stars float64 [96, 128], sky float64 [N, 96, 128])"""
    H, W = SCENE_SHAPE
    rng = np.random.default_rng(seed)
    stars = frame.star_field(SCENE_SHAPE, nstars=40, seed=1)
    yy, xx = np.mgrid[0:H, 0:W]
    sky = np.empty((N, H, W))
    for i in range(N):
        th = 2 * np.pi * i / N
        sky[i] = SKY + AMPLITUDE * (i / (N - 1)) * 2 * (np.cos(th) * (xx / (W - 1) - 0.5) + np.sin(th) * (yy / (H - 1) - 0.5))
    cube = stars[None] + sky + rng.normal(0.0, SCENE_NOISE, (N, H, W))
    for f in TRAIL_FRAMES:
        cube[f, TRAIL_ROW] += TRAIL_ADU
    return cube.astype(F), stars, sky


def box_stats(cube, box, sigma=3.0, maxiters=5):
    """The host's stand-in for ops.local_stats where no device is at hand: per frame and box the clipped (median, std, survivors,
    masked) of frame.clipped_stats - float64 [N, ny, nx, 4]; not bit-pinned to the device kernel."""
    cube = np.asarray(cube)
    bh, bw = (box, box) if np.ndim(box) == 0 else box
    N, H, W = cube.shape
    ny, nx = -(-H // bh), -(-W // bw)
    out = np.zeros((N, ny, nx, 4))
    for i in range(N):
        for j in range(ny):
            for k in range(nx):
                x = np.asarray(cube[i, j * bh:(j + 1) * bh, k * bw:(k + 1) * bw], np.float64).ravel()
                fin = x[np.isfinite(x)]
                out[i, j, k, 3] = bh * bw - fin.size
                if fin.size == 0:
                    out[i, j, k, :2] = np.nan
                    continue
                for _ in range(maxiters):
                    med, sd = np.median(fin), np.std(fin)
                    keep = (fin >= med - sigma * sd) & (fin <= med + sigma * sd)
                    if keep.all():
                        break
                    fin = fin[keep]
                out[i, j, k, :3] = np.median(fin), np.std(fin), fin.size
    return out


def scene_figures(result, cube_shape, stars):
    """What the issue's table reports for one stack of the scene: dict(trail_kept: share of the 2 W trail values the rule kept,
    row_error: mean error along the trail row against stars + 200, rms_off: rms error off the trail row, lost: share of the good
    values the rule removed)."""
    keep = np.asarray(result['keep']).reshape(cube_shape)
    mean = np.asarray(result['mean_f64']).reshape(cube_shape[1:])
    err = mean - (stars + SKY)
    good = np.ones(cube_shape, bool)
    good[list(TRAIL_FRAMES), TRAIL_ROW] = False
    off = np.ones(cube_shape[1], bool)
    off[TRAIL_ROW] = False
    return dict(trail_kept=float(keep[list(TRAIL_FRAMES), TRAIL_ROW].mean()), row_error=float(err[TRAIL_ROW].mean()),
                rms_off=float(np.sqrt((err[off] ** 2).mean())), lost=float((~keep & good).sum() / good.sum()))
