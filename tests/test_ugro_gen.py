"""The generator of tests/test_gpu_ugro_fuzz.py (tests/_ugro_gen.py) held to its promise on any host, from the model
alone: every batch of every seed used has a few hundred frames, at least one run of three or more datagrams — by
adjacency and per flow — and at least one non-member; and a seed always draws the same batch."""
import numpy as np
import pytest

import _ugro
import _ugro_gen as G


@pytest.mark.parametrize("seed", G.SEEDS)
@pytest.mark.parametrize("ipver", [4, 6])
def test_every_drawn_batch_has_a_run_of_three_and_a_non_member(ipver, seed):
    buf, offs, valid, protected = G.draw(seed, ipver)
    n = offs.size - 1
    assert 150 <= n <= 400 and protected >= 4 and valid[:protected].all()
    for model in (_ugro.ugro, _ugro.ugro_flow):
        out = model(buf, offs, valid, ipver)
        assert out["frame_cnt"].max() >= 3, model.__name__
        assert (out["frame_seg"] == _ugro.NONE).sum() >= 1, model.__name__
        assert out["n_super"] < int((out["frame_seg"] != _ugro.NONE).sum())
    assert out["n_super"] <= _ugro.ugro(buf, offs, valid, ipver)["n_super"]  # per flow merges no less
    again = G.draw(seed, ipver)
    assert np.array_equal(again[0], buf) and np.array_equal(again[1], offs) and np.array_equal(again[2], valid)


def test_the_sprinkling_reaches_every_kind_of_non_member():
    """Over the seeds used: frames whose bit the verify clears, frames whose bit is set and which are no members
    (padded, or IPv4 with a zero checksum field), and good frames whose bit was cleared."""
    seen = set()
    for ipver in (4, 6):
        for seed in G.SEEDS:
            buf, offs, valid, _ = G.draw(seed, ipver)
            for i in range(offs.size - 1):
                f = buf[int(offs[i]):int(offs[i + 1])].tobytes()
                member = _ugro.parse(f, ipver) is not None
                seen.add(("valid" if valid[i] else "clear", "member" if member else "other"))
    assert seen == {("valid", "member"), ("valid", "other"), ("clear", "member"), ("clear", "other")}
