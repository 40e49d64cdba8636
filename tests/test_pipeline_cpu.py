"""pipeline.py's host-side pieces without a device: the segment plan against the reference's slices written out as
numbers, and the argument checks of the clip stream and the batched pass, which raise before any device work."""
import random

import pytest
import torch

from rvc_amd.pipeline import VC, Config, segment_plan

WINDOW, T_PAD2, N = 160, 32000, 2_000_000


def test_segment_plan_matches_reference_slices():
    assert segment_plan([], N, WINDOW, T_PAD2) == [(0, 2000000, 0, None)]
    assert segment_plan([607990, 1215777], N, WINDOW, T_PAD2) == [
        (0, 640000, 0, 3999),
        (607840, 1247840, 3799, 7798),
        (1215680, 2000000, 7598, None),
    ]


def test_segment_plan_overlap_and_frames():
    rng = random.Random(5)
    for _ in range(8):
        opt_ts = sorted(rng.sample(range(50_000, N - 50_000), rng.randint(1, 6)))
        segs = segment_plan(opt_ts, N, WINDOW, T_PAD2)
        assert len(segs) == len(opt_ts) + 1 and segs[0][0] == 0 and segs[-1][1] == N and segs[-1][3] is None
        for (a, b, fa, fb), (a1, _, _, _) in zip(segs, segs[1:]):
            assert b - a1 == T_PAD2 + WINDOW
            assert fb == (b - WINDOW) // WINDOW
        for a, _, fa, _ in segs:
            assert a % WINDOW == 0 and fa == a // WINDOW


def stream(vc, audios, **kw):
    return vc.pipeline_device_stream(None, None, 0, audios, 0, "v2", 0.33, **kw)


def test_stream_argument_checks_raise_before_device_work():
    vc = VC(48000, Config("cpu"))
    a, b = torch.zeros(16000), torch.zeros(16160)
    with pytest.raises(ValueError, match="t_max"):
        stream(vc, [a, torch.zeros(vc.t_max - vc.window + 1)])
    with pytest.raises(ValueError, match="equal-length"):
        stream(vc, [a, b], batch=2)
    with pytest.raises(ValueError, match="one seed per clip"):
        stream(vc, [a, a], seeds=[1])
    with pytest.raises(ValueError, match="one host buffer per clip"):
        stream(vc, [a, a], host_out=[torch.zeros(48000)])
    assert stream(vc, []) == []
    assert vc.seed == 0


def test_batch_argument_checks_raise_before_device_work():
    vc = VC(48000, Config("cpu"))
    with pytest.raises(ValueError, match="equal-length"):
        vc.pipeline_device_batch(None, None, 0, [torch.zeros(16000), torch.zeros(16160)], 0, "v2", 0.33)
