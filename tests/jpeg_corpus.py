"""The JPEG files the entropy-decoder tests share (tests/test_jpeg_decode_chunked.py on the host,
tests/test_gpu_jpeg_decode.py on the device): written by PIL (libjpeg-turbo) from fixed seeds, built
once per process, read-only.

  sizes     1x1, 8x8, 17x13, 64x64, 250x131, 256x256
  sampling  4:4:4, 4:2:2, 4:2:0, grey
  quality   50, 75, 95, 100
  content   uniform noise (long codes, many FF 00), flat (about 6 bits per block: more than a hundred
            blocks per subsequence), a small data.synth_image
  tables    standard and optimize=True (custom tables)
  restarts  restart_marker_blocks 1, 2, 7 (7 is no multiple of an MCU row and leaves a short last segment)

check_corpus() asserts what keeps the corpus hard: at the minimum subsequence size a scan of more
than two workgroups of subsequences, an FF 00 pair whose FF is the last byte of a subsequence (its
stuffed zero falls into the next lane's bytes) and one that straddles a 4-KiB unstuffing chunk; at
the default size a scan shorter than one subsequence."""
import functools
import io

import numpy as np
from PIL import Image, ImageFile

SUBSEQ_MIN, SUBSEQ_DEFAULT, LANES, CHUNK = 64, 512, 256, 4096
SAMPLING = {"444": 0, "422": 1, "420": 2}


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat(h, w, seed):
    return np.full((h, w, 3), (seed * 37) % 256, dtype=np.uint8)


def synth(h, w, seed):
    from mx_det.data import synth_image
    return synth_image(seed, H=h, W=w)


CONTENT = {"noise": noise, "flat": flat, "synth": synth}


def pil_jpeg(img, quality, sampling, optimize=False, restart=0):
    buf = io.BytesIO()
    kw = {"format": "JPEG", "quality": quality, "optimize": optimize}
    if restart:
        kw["restart_marker_blocks"] = restart
    # the encoder gets one buffer for the whole file when optimize is on: PIL sizes it from the pixel
    # count, which a noise image with restart markers exceeds
    block, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, max(ImageFile.MAXBLOCK, 8 * img.size + 4096)
    try:
        if sampling == "grey":
            Image.fromarray(img[..., 1]).save(buf, **kw)
        else:
            Image.fromarray(img).save(buf, subsampling=SAMPLING[sampling], **kw)
    finally:
        ImageFile.MAXBLOCK = block
    return buf.getvalue()


# (content, H, W, seed, quality, sampling, optimize, restart_marker_blocks)
SPECS = [
    ("noise", 1, 1, 1, 75, "420", False, 0),      # one MCU, a scan of a few bytes
    ("flat", 1, 1, 2, 50, "grey", False, 0),
    ("noise", 8, 8, 3, 95, "444", False, 0),
    ("noise", 8, 8, 4, 100, "grey", True, 0),
    ("synth", 17, 13, 5, 75, "420", False, 0),
    ("noise", 17, 13, 6, 100, "422", True, 0),
    ("noise", 17, 13, 7, 95, "444", False, 1),
    ("noise", 64, 64, 8, 100, "444", False, 0),   # 98 or so FF 00 pairs, more than two workgroups at 64 bits
    ("noise", 64, 64, 9, 95, "420", True, 0),
    ("noise", 64, 64, 10, 50, "422", False, 2),
    ("noise", 64, 64, 11, 100, "grey", False, 7),
    ("flat", 64, 64, 12, 75, "420", False, 0),
    ("flat", 64, 64, 13, 95, "444", True, 0),
    ("synth", 64, 64, 14, 95, "420", False, 7),
    ("synth", 250, 131, 15, 75, "420", False, 0),
    ("noise", 250, 131, 16, 95, "422", False, 7),
    ("noise", 250, 131, 17, 100, "444", True, 2),
    ("flat", 250, 131, 18, 50, "grey", False, 1),
    ("synth", 250, 131, 19, 100, "grey", True, 0),
    ("flat", 256, 256, 20, 95, "420", False, 0),  # 1536 blocks in fewer than 20 subsequences of 512 bits
    ("flat", 256, 256, 21, 100, "444", False, 7),
    ("synth", 256, 256, 22, 95, "420", True, 1),
    ("noise", 256, 256, 23, 75, "420", False, 0),
    ("noise", 256, 256, 24, 100, "444", False, 0),  # some 190 KiB: FF 00 pairs across 4-KiB chunk boundaries
    ("noise", 256, 256, 25, 100, "420", True, 7),
    ("noise", 256, 256, 26, 50, "422", True, 2),
]


def spec_id(s):
    return "%s-%dx%d-q%d-%s%s%s" % (s[0], s[1], s[2], s[4], s[5], "-opt" if s[6] else "", "-r%d" % s[7] if s[7] else "")


IDS = [spec_id(s) for s in SPECS]


@functools.lru_cache(maxsize=None)
def jpeg_file(i):
    """The bytes of corpus file i."""
    content, h, w, seed, q, sampling, opt, rst = SPECS[i]
    return pil_jpeg(CONTENT[content](h, w, seed), q, sampling, opt, rst)


@functools.lru_cache(maxsize=None)
def reference(i):
    """(info, coefficients) of file i by the sequential host decoder; read-only."""
    from mx_det import jpeg
    info, coefs = jpeg.decode_coefs(jpeg_file(i))
    coefs.setflags(write=False)
    return info, coefs


def scan_layout(data, scan_off):
    """Restart segments of the scan as the decoders cut it: a list of (raw index of every kept byte,
    raw index of every stuffed FF) per segment; indices count from scan_off."""
    s = np.frombuffer(data, dtype=np.uint8)[scan_off:]
    segs, kept, stuffed, live, i = [], [], [], True, 0
    while i < len(s):
        if s[i] == 0xFF and i + 1 < len(s) and s[i + 1] != 0:
            if 0xD0 <= s[i + 1] <= 0xD7:
                segs.append((kept, stuffed))
                kept, stuffed, live = [], [], True
            else:
                live = False
            i += 2
            continue
        if live:
            kept.append(i)
            if s[i] == 0xFF:
                stuffed.append(i)
        i += 2 if s[i] == 0xFF else 1
    segs.append((kept, stuffed))
    return segs


@functools.lru_cache(maxsize=None)
def check_corpus():
    """The conditions of the module docstring; returns the figures."""
    from mx_det import jpeg
    most_subseq, lane_straddles, chunk_straddles, shortest = 0, 0, 0, 1 << 60
    for i in range(len(SPECS)):
        data = jpeg_file(i)
        off = jpeg.parse(data).scan_off
        bits = 0
        for kept, stuffed in scan_layout(data, off):
            bits += 8 * len(kept)
            pos = {raw: k for k, raw in enumerate(kept)}
            lane_straddles += sum((pos[raw] + 1) * 8 % SUBSEQ_MIN == 0 for raw in stuffed)
            # the file goes to a 16-byte aligned device buffer: chunks are cut at aligned addresses
            chunk_straddles += sum((raw + off % 16) % CHUNK == CHUNK - 1 for raw in stuffed)
        most_subseq = max(most_subseq, bits // SUBSEQ_MIN)
        shortest = min(shortest, bits)
    assert most_subseq > 2 * LANES, most_subseq
    assert lane_straddles > 0 and chunk_straddles > 0, (lane_straddles, chunk_straddles)
    assert shortest < SUBSEQ_DEFAULT, shortest
    return most_subseq, lane_straddles, chunk_straddles, shortest
