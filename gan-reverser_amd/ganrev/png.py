"""PNG files with the standard library alone (zlib, struct): what ganrev.render's pictures are saved as.

The reference saves JPEG through Torch's `image` rock (image.save); JPEG is lossy and its encoder is not restated here, so the pictures
are written as 8-bit PNG instead - lossless, which lets a test read a file back and compare it byte for byte with the grid it came from.

    write_png(path, u8)     u8: uint8 array [H x W x 1] (or [H x W]) -> grayscale, [H x W x 3] -> RGB, [H x W x 4] -> RGBA; filter 0 on
                            every scanline
    read_png(path)          8-bit grayscale, RGB or RGBA, non-interlaced, any of the five scanline filters -> uint8 [H x W x 1 | 3 | 4]

ganrev.dataset decodes a folder of .png files with read_png (dataset.lua:111,149: image.load); RGBA is there for that.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data):
    """one PNG chunk: length, type, data, CRC-32 of type + data"""
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(u8, level=6):
    u8 = np.asarray(u8)
    if u8.dtype != np.uint8:
        raise ValueError(f"write_png: uint8 pixels, not {u8.dtype}")
    if u8.ndim == 2:
        u8 = u8[:, :, None]
    if u8.ndim != 3 or u8.shape[2] not in (1, 3, 4) or u8.shape[0] < 1 or u8.shape[1] < 1:
        raise ValueError(f"write_png: [H x W x 1], [H x W x 3] or [H x W x 4], not {u8.shape}")
    h, w, c = u8.shape
    raw = np.zeros((h, 1 + w * c), np.uint8)                  # filter byte 0 (None) in front of every scanline
    raw[:, 1:] = u8.reshape(h, w * c)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + chunk(b"IEND", b"")


def write_png(path, u8):
    data = encode_png(u8)
    with open(path, "wb") as f:
        f.write(data)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def decode_png(data):
    if data[:8] != SIGNATURE:
        raise ValueError("read_png: not a PNG file")
    pos, ihdr, idat = 8, None, []
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"read_png: bad CRC in chunk {kind!r}")
        pos += 12 + n
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if ihdr is None:
        raise ValueError("read_png: no IHDR chunk")
    w, h, depth, ctype, comp, flt, interlace = ihdr
    if depth != 8 or ctype not in (0, 2, 6) or comp != 0 or flt != 0 or interlace != 0:
        raise ValueError(f"read_png: only 8-bit gray / RGB / RGBA, non-interlaced (depth {depth}, colour type {ctype}, interlace {interlace})")
    c = {0: 1, 2: 3, 6: 4}[ctype]
    stride = w * c
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (stride + 1):
        raise ValueError(f"read_png: {len(raw)} bytes of scanlines, expected {h * (stride + 1)}")
    out = np.zeros((h, stride), np.uint8)
    prev = bytearray(stride)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = bytearray(raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        if ft == 1:                                           # Sub
            for i in range(c, stride):
                line[i] = (line[i] + line[i - c]) & 255
        elif ft == 2:                                         # Up
            for i in range(stride):
                line[i] = (line[i] + prev[i]) & 255
        elif ft == 3:                                         # Average
            for i in range(stride):
                line[i] = (line[i] + (((line[i - c] if i >= c else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:                                         # Paeth
            for i in range(stride):
                line[i] = (line[i] + _paeth(line[i - c] if i >= c else 0, prev[i], prev[i - c] if i >= c else 0)) & 255
        elif ft != 0:
            raise ValueError(f"read_png: unknown filter type {ft} on scanline {y}")
        out[y] = np.frombuffer(bytes(line), np.uint8)
        prev = line
    return out.reshape(h, w, c)


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())
