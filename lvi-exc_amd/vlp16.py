"""VLP-16 data packets for tests and demos: the inverse of the unpacking lvx_set_scans_vlp16 does (lvi-exc_amd/csrc/lvx_vlp16.h).  Kept out of synth.py, which the
benchmark imports.

A packet is 1206 bytes, little-endian: 12 blocks of {uint16 header 0xEEFF, uint16 rotation [1/100 deg], 32 x {uint16 distance [2 mm], uint8 intensity}} and 6 trailer
bytes (a 4-byte counter and 2 status bytes, which the unpacking never reads).  The 32 returns of a block are two firings of the 16 lasers; laser `dsr` lands in row
ROW_OF_DSR[dsr] of the organised scan, firing f of block b of packet p in column 24 p + 2 b + f."""
import numpy as np

PACKET_BYTES = 1206
BLOCKS = 12
COLS = 24                                     # columns per packet
HEADER = 0xEEFF
DISTANCE_RESOLUTION = 0.002                   # metres per unit
ROW_OF_DSR = np.array([15, 7, 14, 6, 13, 5, 12, 4, 11, 3, 10, 2, 9, 1, 8, 0])
DSR_OF_ROW = np.argsort(ROW_OF_DSR)
# elevation of the lasers [rad], by dsr: -15, 1, -13, 3, ... degrees
VERT_ANGLE = np.deg2rad(np.array([-15, 1, -13, 3, -11, 5, -9, 7, -7, 9, -5, 11, -3, 13, -1, 15], np.float64))


def quantise(ranges_m):
    """Ranges [m] -> the packet's uint16 units (2 mm, rounded to nearest, clipped); a non-finite range is 0 = no return."""
    r = np.asarray(ranges_m, np.float64)
    q = np.rint(np.where(np.isfinite(r), r, 0.0) / DISTANCE_RESOLUTION)
    return np.clip(q, 0, 65535).astype(np.uint16)


def encode_packets(ranges_m, intensity, rotation0, rotation_step):
    """Well-formed packets of one scan.  ranges_m [16][C]: ranges in metres as the ORGANISED scan holds them (row, column), C a multiple of 24; intensity: the same
    shape or a scalar, 0 .. 255.  Block k of the scan (k = 0 .. C / 2 - 1) carries rotation (rotation0 + k * rotation_step) mod 36000.  Returns C / 24 * 1206 bytes."""
    raw = quantise(ranges_m)
    if raw.ndim != 2 or raw.shape[0] != 16 or raw.shape[1] % COLS:
        raise ValueError("ranges_m: [16][C] with C a multiple of 24")
    inten = np.broadcast_to(np.asarray(intensity), raw.shape)
    if (inten < 0).any() or (inten > 255).any():
        raise ValueError("intensity: 0 .. 255")
    inten = inten.astype(np.uint8)
    n_blocks = raw.shape[1] // 2
    pk = np.zeros((n_blocks // BLOCKS, PACKET_BYTES), np.uint8)
    rot = ((int(rotation0) + np.arange(n_blocks, dtype=np.int64) * int(rotation_step)) % 36000).astype(np.uint16)
    blocks = np.zeros((n_blocks, 100), np.uint8)                # [block of the scan][100 bytes]
    blocks[:, 0], blocks[:, 1] = HEADER & 255, HEADER >> 8
    blocks[:, 2], blocks[:, 3] = rot & 255, rot >> 8
    data = np.zeros((n_blocks, 2, 16, 3), np.uint8)             # [block][firing][dsr][3 bytes]
    by_dsr = raw[ROW_OF_DSR].reshape(16, n_blocks, 2).transpose(1, 2, 0)   # [block][firing][dsr]
    data[..., 0], data[..., 1] = by_dsr & 255, by_dsr >> 8
    data[..., 2] = inten[ROW_OF_DSR].reshape(16, n_blocks, 2).transpose(1, 2, 0)
    blocks[:, 4:] = data.reshape(n_blocks, 96)
    pk[:, :BLOCKS * 100] = blocks.reshape(len(pk), BLOCKS * 100)
    pk[:, 1200:1204] = np.arange(len(pk), dtype="<u4").view(np.uint8).reshape(-1, 4)   # the trailer's counter; status bytes stay 0
    return pk.tobytes()
