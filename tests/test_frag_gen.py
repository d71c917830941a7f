"""The fuzz generator of tests/_frag_gen.py held to a floor: every seed's model output holds at least one complete
datagram of three or more fragments, one leftover and one non-member, and one frame of each fragmentation status — so no
seed of tests/test_gpu_frag_fuzz.py is vacuous."""
import numpy as np
import pytest

import _frag as F
import _frag_gen as GEN


@pytest.mark.parametrize("seed", GEN.SEEDS)
def test_no_seed_is_vacuous(seed):
    buf, offs, mtu = GEN.frag_batch(seed)
    _, _, _, _, status = F.frag(buf, offs, mtu)
    assert {F.PASS, F.CUT, F.DF, F.BAD} <= set(status.tolist())
    buf, offs = GEN.reasm_batch(seed)
    o = F.reasm(buf, offs)
    n = offs.size - 1
    member = np.unpackbits(o["is_frag"].view(np.uint8), bitorder="little")[:n].astype(bool)
    assert o["n_out"] >= 1 and o["frag_cnt"].max() >= 3
    assert ((o["frame_seg"] == F.NONE) & member).any(), "no leftover"
    assert (~member).any(), "no non-member"
    t = GEN.tune(np.random.default_rng(seed))
    assert t is None or set(t) == {"blocks_per_cu", "run_segs", "rows"}
