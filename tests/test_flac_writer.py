"""CPU: the test writer (tests/flac_writer.py) pinned to the MD5-checked Python decoder, and the library's frame index (wlx_flac_probe,
host only) pinned to both: the writer's CRC-8 / CRC-16 are the library's, and the library's are a real encoder's (jfk_head.flac)."""
import os

import numpy as np
import pytest

from whisperlive_amd import audio_io

from . import flac_cases as FC

JFK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jfk_head.flac")
CASES = FC.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_written_stream_decodes_to_the_integers_given_and_probes_with_the_right_counts(case):
    x, sr = audio_io.read_flac(case["data"], verify_md5=True)             # raises unless the decode matches the MD5 the writer stored
    got = np.round(x.astype(np.float64) * (1 << (case["bps"] - 1))).astype(np.int64)
    assert sr == case["rate"] and np.array_equal(got, case["pcm"])
    info = audio_io.flac_probe(case["data"])
    assert (info.sample_rate, info.channels, info.bits_per_sample, info.total_samples, info.n_frames, info.max_blocksize) == \
        (case["rate"], case["pcm"].shape[1], case["bps"], case["pcm"].shape[0], len(case["frames"]), max(case["blocks"]))
    from whisperlive_amd.engine import resample_supported
    assert info.served == int(resample_supported(case["rate"], case["pcm"].shape[1]))


def test_probe_indexes_a_real_encoders_file():
    with open(JFK, "rb") as f:
        info = audio_io.flac_probe(f.read())
    assert (info.n_frames, info.total_samples, info.bits_per_sample, info.channels, info.sample_rate, info.served) == \
        (32, 147456, 24, 2, 44100, 1)
