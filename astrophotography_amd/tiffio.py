"""Baseline TIFF 6.0 writer for the colour composites (ApComposite): little-endian, uncompressed, chunky RGB, 8 or 16 bits per
channel, with the ImageDescription, Software and Copyright tags STIFF sets.  Pure Python; classic TIFF only - its offsets are
32 bits wide, so an image whose file would reach 4 GiB is refused (there is no BigTIFF support).

File layout: header (8 bytes), the IFD, the values that do not fit an IFD entry, then the pixel data as strips of whole rows.
"""
import os
import struct

import numpy as np

SOFTWARE = 'astrophotography_amd ApComposite'
STRIP_BYTES = 1 << 20                   # strips of about 1 MiB (whole rows)
MAX_FILE = 1 << 32

_BYTE, _ASCII, _SHORT, _LONG, _RATIONAL = 1, 2, 3, 4, 5
_SIZE = {_BYTE: 1, _ASCII: 1, _SHORT: 2, _LONG: 4, _RATIONAL: 8}


def _ascii(text):
    return str(text).encode('ascii', 'replace') + b'\0'


def _pack(ftype, values):
    if ftype == _ASCII:
        return values
    if ftype == _RATIONAL:
        return b''.join(struct.pack('<II', n, d) for n, d in values)
    return struct.pack('<%d%s' % (len(values), {_BYTE: 'B', _SHORT: 'H', _LONG: 'I'}[ftype]), *values)


def layout(height, width, bits, description='', copyright='', software=SOFTWARE):
    """(head bytes, data offset, data bytes) of the file of a [height][width][3] image: `head` is everything in front of the
    pixel data.  Raises ValueError for a shape or depth TIFF cannot hold and for files of 4 GiB or more."""
    height, width, bits = int(height), int(width), int(bits)
    if bits not in (8, 16):
        raise ValueError('TIFF output has 8 or 16 bits per channel, got %r' % (bits,))
    if height < 1 or width < 1:
        raise ValueError('cannot write an image of %d x %d' % (height, width))
    row_bytes = width * 3 * (bits // 8)
    nbytes = row_bytes * height
    rows_per_strip = max(1, min(height, STRIP_BYTES // row_bytes))
    nstrips = (height + rows_per_strip - 1) // rows_per_strip
    counts = [min(rows_per_strip, height - s * rows_per_strip) * row_bytes for s in range(nstrips)]
    # (tag, type, values); the strip offsets are filled in once the size of the head is known
    tags = [(256, _LONG, [width]), (257, _LONG, [height]), (258, _SHORT, [bits] * 3), (259, _SHORT, [1]), (262, _SHORT, [2]),
            (270, _ASCII, _ascii(description)), (273, _LONG, None), (274, _SHORT, [1]), (277, _SHORT, [3]),
            (278, _LONG, [rows_per_strip]), (279, _LONG, counts), (282, _RATIONAL, [(72, 1)]), (283, _RATIONAL, [(72, 1)]),
            (284, _SHORT, [1]), (296, _SHORT, [2]), (305, _ASCII, _ascii(software)), (33432, _ASCII, _ascii(copyright))]
    ifd_bytes = 2 + 12 * len(tags) + 4
    extra = 8 + ifd_bytes
    sizes = []
    for tag, ftype, values in tags:
        n = nstrips if values is None else len(values)
        sizes.append(n * _SIZE[ftype])
        if sizes[-1] > 4:
            extra += sizes[-1] + (sizes[-1] & 1)                # values start on a word boundary
    data_offset = (extra + 3) & ~3
    if data_offset + nbytes >= MAX_FILE:
        raise ValueError('a %d x %d image at %d bits needs a TIFF file of %d bytes: 4 GiB or more cannot be written (classic TIFF '
                         'has 32-bit offsets; BigTIFF is not supported)' % (width, height, bits, data_offset + nbytes))
    offsets, at = [], data_offset
    for c in counts:
        offsets.append(at)
        at += c
    entries, blob, pos = [], b'', 8 + ifd_bytes
    for (tag, ftype, values), size in zip(tags, sizes):
        raw = _pack(ftype, offsets if values is None else values)
        count = len(raw) // _SIZE[ftype]
        if size <= 4:
            entries.append(struct.pack('<HHI', tag, ftype, count) + raw.ljust(4, b'\0'))
        else:
            entries.append(struct.pack('<HHII', tag, ftype, count, pos + len(blob)))
            blob += raw + (b'\0' if size & 1 else b'')
    head = b'II' + struct.pack('<HI', 42, 8) + struct.pack('<H', len(tags)) + b''.join(entries) + struct.pack('<I', 0) + blob
    assert len(head) == extra
    return head.ljust(data_offset, b'\0'), data_offset, nbytes


def _put(path, head, data_bytes):
    tmp = str(path) + '.tmp%d' % os.getpid()
    with open(tmp, 'wb') as f:
        f.write(head)
        f.write(data_bytes)
    os.replace(tmp, path)


def write(path, image, description='', copyright='', software=SOFTWARE, overwrite=True):
    """Writes a host array [H][W][3] of uint8 or uint16 as an RGB TIFF."""
    if os.path.exists(path) and not overwrite:
        raise OSError("File '%s' already exists." % path)
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype not in (np.uint8, np.uint16):
        raise ValueError('image must be [H][W][3] uint8 or uint16, got %s %s' % (image.shape, image.dtype))
    head, _, nbytes = layout(image.shape[0], image.shape[1], 8 * image.dtype.itemsize, description, copyright, software)
    data = np.ascontiguousarray(image, dtype=image.dtype.newbyteorder('<'))
    assert data.nbytes == nbytes
    _put(path, head, memoryview(data).cast('B'))


def write_device(path, tensor, description='', copyright='', software=SOFTWARE, overwrite=True, pool=None):
    """Writes a device tensor [H][W][3] of uint8 or uint16 as an RGB TIFF, through the pinned staging buffers fitsio.write_device
    uses.  pool: a fitsio.WritePool - the file is written by one of its threads after this call returned (pool.wait() before
    reading it)."""
    import torch
    from . import fitsio
    if os.path.exists(path) and not overwrite:
        raise OSError("File '%s' already exists." % path)
    if tensor.dim() != 3 or tensor.shape[2] != 3 or tensor.dtype not in (torch.uint8, torch.uint16):
        raise ValueError('tensor must be [H][W][3] uint8 or uint16, got %s %s' % (tuple(tensor.shape), tensor.dtype))
    if not tensor.is_cuda:
        host = tensor.numpy() if tensor.dtype == torch.uint8 else tensor.view(torch.int16).numpy().view(np.uint16)
        return write(path, host, description, copyright, software, overwrite)
    head, _, nbytes = layout(tensor.shape[0], tensor.shape[1], 8 * tensor.element_size(), description, copyright, software)
    payload = tensor.contiguous().view(torch.uint8).reshape(-1)
    slot = pool.staging(nbytes) if pool is not None else None
    host = slot[0][:nbytes] if slot is not None else fitsio._staging(nbytes)
    host.copy_(payload, non_blocking=True)
    torch.cuda.current_stream().synchronize()

    def put():
        _put(path, head, memoryview(host.numpy()))

    if pool is not None:
        pool.submit(slot, put)
    else:
        put()
