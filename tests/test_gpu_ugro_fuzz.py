"""UDP receive coalescing against its model on seeded random batches (tests/_ugro_gen.py): flows cut as UDP
segmentation offload cuts them, interleaved at random, with corrupt, padded and zero-checksum frames and clear valid
bits sprinkled in. Each batch runs both forms with the default and with small tunes — every output array and the
untouched regions — and through the device round trip verify → coalesce → segmentation offload.
tests/test_ugro_gen.py shows on any host that every batch drawn here has a run of three or more frames and a
non-member."""
import numpy as np
import pytest

import _udp
import _ugro
import _ugro_gen as G
import _ugro_gpu as GPU
from _gpu import setup_gpu

pytestmark = pytest.mark.gpu

TUNES = (None, dict(run_segs=16, blocks_per_cu=1, rows=1), dict(run_segs=33, blocks_per_cu=2, rows=2))


@pytest.mark.parametrize("seed", G.SEEDS)
@pytest.mark.parametrize("ipver", [4, 6])
def test_fuzz_both_forms_and_the_round_trip(ipver, seed):
    setup_gpu()
    buf, offs, valid, _ = G.draw(seed, ipver)
    n = offs.size - 1
    for flow in (False, True):
        o = GPU.check(buf, offs, valid, ipver, TUNES, f"seed={seed}", flow=flow)
        assert o["frame_cnt"].max() >= 3 and (o["frame_seg"] == _ugro.NONE).any()
    # the device verify's own mask, less the bits the generator cleared: the members are the model's members
    rx, _, _ = _udp.rx_expected(ipver, buf, offs)
    members = int((_ugro.ugro(buf, offs, valid, ipver)["frame_seg"] != _ugro.NONE).sum())
    for flow in (False, True):
        for tune in TUNES[:2]:
            ps = GPU.assert_round_trip(buf, offs, ipver, tune=tune, flow=flow, keep=valid | ~rx, members=members,
                                       what=f"seed={seed}")
            assert len(set(ps.tolist())) == members <= n
