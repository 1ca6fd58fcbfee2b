"""Host helpers for coarse meshes of per-box statistics (a few hundred float64 numbers): what the sky-background model
(core/ApMeasureBackground.py) and the local normalisation of a stack (ops.local_normalization) do to the boxes they cannot use.
Plain NumPy; nothing here touches the device."""
import numpy as np


def fill_excluded(mesh, good, n_neighbors=10, power=1.0):
    """Background2D._interpolate_meshes: inverse-distance weighting over the k nearest good boxes."""
    ny, nx = mesh.shape
    gy, gx = np.nonzero(good)
    vals = mesh[good]
    out = mesh.copy()                       # a good box is its own nearest neighbour at distance 0: it keeps its value
    k = min(n_neighbors, len(vals))
    for y, x in zip(*np.nonzero(~good)):
        d = np.hypot(gy - y, gx - x)
        order = np.argsort(d, kind='stable')[:k]
        w = 1.0 / d[order] ** power
        out[y, x] = np.sum(w * vals[order]) / np.sum(w)
    return out


def nanmedian_filter(mesh, size):
    """Background2D._filter_meshes: nanmedian over a size x size window, NaN beyond the mesh."""
    if size <= 1:
        return mesh
    h = size // 2
    ny, nx = mesh.shape
    pad = np.full((ny + 2 * h, nx + 2 * h), np.nan)
    pad[h:h + ny, h:h + nx] = mesh
    win = np.stack([pad[dy:dy + ny, dx:dx + nx] for dy in range(size) for dx in range(size)], 0)
    return np.nanmedian(win, axis=0)
