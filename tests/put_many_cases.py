"""What the wlx_pcm_put_many tests share: synthetic FLAC streams of a given frame count, and a stream with a frame that passes the host
index and fails in the decoder."""
import numpy as np

from . import flac_cases as FC
from . import flac_writer as FW


def flac_stream(n_frames, block, bps, ch, seed, assignment=FW.INDEPENDENT, rate=16000):
    rng = np.random.RandomState(seed)
    pcm = FC.smooth(rng, block * (n_frames - 1) + max(1, block // 3), ch, bps)           # a short last frame
    blocks = FW.split_blocks(pcm.shape[0], block)
    assert len(blocks) == n_frames
    sub = lambda f, c: FC.fit({"type": "fixed", "order": 2, "k": min(14, max(5, bps - 8))}, blocks[f])          # noqa: E731
    return FW.encode_stream(pcm, rate, bps, blocks, subframe=sub, assignment=assignment), pcm


def broken_frame_stream(rate=16000, seed=11):
    """a mono 16-bit stream of 5 frames of 64 whose second frame passes the host index (sync, CRC-8, number, CRC-16 all right) and fails in
    the decoder: the padding bit of its subframe header is set, and the CRC-16 is the one of the bytes as they are -> (bytes, pcm)"""
    rng = np.random.RandomState(seed)
    pcm = FC.smooth(rng, 64 * 5, 1, 16)
    frames = FW.encode_frames(pcm, rate, 16, [64] * 5, subframe={"type": "fixed", "order": 1, "k": 6})
    f = bytearray(frames[1])
    f[len(FW.frame_header(64, rate, 1, 16, 1, False, FW.INDEPENDENT))] |= 0x80
    f[-2:] = FW.crc16(bytes(f[:-2])).to_bytes(2, "big")
    frames[1] = bytes(f)
    return FW.metadata(FW.streaminfo(pcm, rate, 16, 64, 64)) + b"".join(frames), pcm
