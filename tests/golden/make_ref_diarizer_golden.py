"""Generate tests/golden/ref_diarizer_golden.json: what the reference's OWN SpeakerDiarizer answers on the seeded clustering
scenarios of tests/test_spk_host.py.

Run with a checkout of the reference:  python tests/golden/make_ref_diarizer_golden.py REFERENCE_ROOT

whisper_live/diarization.py is loaded by path (it imports only numpy at module level; pyannote.audio is never touched, because
`_compute_embedding` is overridden to replay the scenario's seeded unit vectors, None entries included). Per scenario the fixture
keeps the outputs of every operation (labels, None, enrolment results, "reset") and the final centroids in insertion order.
Only DATA is stored."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.test_spk_host import GOLDEN, N_SCENARIOS, replay, scenario  # noqa: E402


def main():
    path = os.path.join(sys.argv[1] if len(sys.argv) > 1 else ".", "whisper_live", "diarization.py")
    spec = importlib.util.spec_from_file_location("_ref_diarization", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Replayed(mod.SpeakerDiarizer):
        def __init__(self, feed, **kw):
            super().__init__(**kw)
            self.feed = feed

        def _compute_embedding(self, audio_np, sample_rate=16000):
            return self.feed.pop(0)

    out = []
    for i in range(N_SCENARIOS):
        kw, ops = scenario(i)
        feed = []
        d = Replayed(feed, **kw)
        res = replay(d, ops, feed)
        out.append({"out": res, "centroids": {k: [round(float(x), 8) for x in v] for k, v in d.speakers.items()}})
    with open(GOLDEN, "w") as f:
        json.dump({"n": N_SCENARIOS, "scenarios": out}, f, separators=(",", ":"))
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
