"""The far layouts of tests/_far.py discriminate, shown without a GPU: for each wrap placement and each pass the
project's own model gives a different result on the low-32 twin — the batch as a kernel that kept only the low word of
the span's length would see it — than on the compact twin the GPU tests take their expected values from. So a
truncating kernel cannot pass tests/test_gpu_far_offsets.py. Plus the helper's invariants: D a multiple of 2^17, every
frame's bytes and its address modulo 128 equal in the twin and in the far layout, exactly one frame across byte 2^32 in
the straddle placements.

Where the contract gives a zero-length frame and a 2^32-byte span of junk the same outputs (wrap_empty under the IPv6
receive pass, both coalescing calls and the NAT rewrite: neither is well-formed, neither is a member, and no output
carries more than that) there is nothing a length-truncating kernel could get wrong, and the test pins exactly that:
the two models agree. What holds those passes there is the address arithmetic behind the span, which the far frames'
expected values check on the GPU; their length classification is held by wrap_frame."""
import numpy as np
import pytest

import _far
import _gro

MIX = "small"  # the placements' arithmetic does not depend on the far frames' sizes; the GPU tests run both mixes


def _bits(mask, n):
    return _gro.valid_bits(mask, n)


def _check_invariants(r):
    assert r.D % (1 << 17) == 0 and r.D == r.S - r.S_twin and (1 << 17) <= r.S_twin < (1 << 18)
    assert r.S % (1 << 17) == r.S_twin % (1 << 17)
    o, fo = r.offs.astype(object), r.far_offs.astype(object)
    assert all(fo[i] <= fo[i + 1] for i in range(r.n))
    assert fo[r.span + 1] - fo[r.span] == r.S and all(fo[i] == o[i] for i in range(r.span + 1))
    for i in range(r.span + 1, r.n + 1):
        assert fo[i] - o[i] == r.D and fo[i] % 128 == o[i] % 128
    # every frame's bytes: the three ranges carry the twin's bytes to the frames' device addresses
    (d0, t0, n0), (d1, t1, n1), (d2, t2, n2) = r.ranges
    assert (d0, t0) == (0, 0) and n0 == o[r.span] and (d1, t1, n1) == (o[r.span], o[r.span], _far.HEAD)
    assert d2 == fo[r.span + 1] and t2 == o[r.span + 1] and d2 + n2 == fo[-1] + 3 and t2 + n2 == r.buf.size
    assert not r.buf[t1 + n1:t2].any() or r.marks  # the rest of the span is zero
    assert d2 + n2 <= _far.ARENA
    across = _far.crossing(r.far_offs)
    if r.placement[0] == "straddle":
        assert fo[r.span + 1] == _far.TWO32 - _far.STRADDLE_BACK + r.placement[1]
        assert len(across) == 1 and across[0] > r.span
        assert sum(1 for i in range(r.n) if fo[i] <= _far.TWO32 < fo[i + 1]) == 1
        assert all(fo[i] > _far.TWO32 for i in range(across[0] + 1, r.n + 1))
    else:
        assert across == [r.span] and fo[r.span + 1] >= _far.TWO32
        assert r.low_offs.astype(object)[r.span + 1] - r.low_offs.astype(object)[r.span] == r.S % _far.TWO32
        lo = r.low_offs.astype(object)
        for i in range(r.n):  # the low-32 twin holds the same frames but for the span
            if i != r.span:
                assert r.low_buf[lo[i]:lo[i + 1]].tobytes() == r.buf[o[i]:o[i + 1]].tobytes()


@pytest.mark.parametrize("placement", _far.PLACEMENTS, ids=_far.pid)
def test_far_layout_invariants(placement):
    for mix in _far.MIXES:
        _check_invariants(_far.rx_batch(4, placement, mix))
        _check_invariants(_far.rx_batch(6, placement, mix))
        _check_invariants(_far.parse_batch(placement, mix))
        _check_invariants(_far.nat_batch(4, placement, mix)[0])
    _check_invariants(_far.csum_batch(placement, MIX))
    for flow in (False, True):
        _check_invariants(_far.gro_batch(4, placement, MIX, flow)[0])
        _check_invariants(_far.gro_batch(6, placement, MIX, flow)[0])


def test_far_markers_keep_value_and_parity():
    for placement in _far.PLACEMENTS:
        r = _far.csum_batch(placement, MIX)
        assert len(r.marks) >= 6
        s0 = int(r.offs[r.span])
        for d, t, b in r.marks:
            assert (d - t) % 2 == 0 and r.buf[t:t + 2].tobytes() == b and any(b)
            assert s0 + _far.HEAD <= d and d + 2 <= s0 + r.S and s0 + _far.HEAD <= t and t + 2 <= s0 + r.S_twin
        rel = [d - s0 for d, _, _ in r.marks]
        assert any(x < (1 << 31) <= x + 4 for x in rel) and any(x > (1 << 31) for x in rel) and any(x % 2 for x in rel)
        assert any(r.S - x <= 256 for x in rel)
        if placement[0] != "straddle":
            ab = [d for d, _, _ in r.marks]
            assert any(a + 2 <= _far.TWO32 for a in ab) and any(a >= _far.TWO32 for a in ab)
            assert any(a < _far.TWO32 < a + 2 for a in ab)


def test_build_slots_one_frame_across():
    rng = np.random.default_rng(5)
    start, twin = _far.build_slots(rng.integers(10, 300, _far.BUILD_NEAR + _far.BUILD_FAR) * 4)
    assert _far.crossing(start) != [] and not (start & np.uint64(3)).any()
    assert np.array_equal(start[:_far.BUILD_NEAR], twin[:_far.BUILD_NEAR])
    assert (start[_far.BUILD_NEAR:] - twin[_far.BUILD_NEAR:] == np.uint64(_far.BUILD_D)).all()
    assert int(twin[_far.BUILD_NEAR - 1]) < int(twin[_far.BUILD_NEAR]) and _far.BUILD_D % (1 << 17) == 0


@pytest.mark.parametrize("ipver", [4, 6])
def test_rx_wrap_frame_discriminates(ipver):
    r = _far.rx_batch(ipver, ("wrap_frame", 0), MIX)
    want, low = _far.rx_model(ipver, r.buf, r.offs), _far.rx_model(ipver, r.low_buf, r.low_offs)
    assert not _bits(want[0], r.n)[r.span] and _bits(low[0], r.n)[r.span]  # the mask bit of the span
    assert want[-1][r.span] == 0 and low[-1][r.span] == 0xFFFF             # its TCP raw sum
    keep = np.arange(r.n) != r.span
    assert all(np.array_equal(w[keep], lw[keep]) for w, lw in zip(want[1:], low[1:]))


def test_rx4_wrap_empty_discriminates():
    r = _far.rx_batch(4, ("wrap_empty", 0), MIX)
    want, low = _far.rx_model(4, r.buf, r.offs), _far.rx_model(4, r.low_buf, r.low_offs)
    assert want[1][r.span] != 0 and low[1][r.span] == 0  # the header's raw sum: a header is there, an empty frame has none
    assert not _bits(want[0], r.n)[r.span] and not _bits(low[0], r.n)[r.span]


def test_rx6_wrap_empty_has_nothing_to_tell():
    r = _far.rx_batch(6, ("wrap_empty", 0), MIX)
    want, low = _far.rx_model(6, r.buf, r.offs), _far.rx_model(6, r.low_buf, r.low_offs)
    assert all(np.array_equal(w, lw) for w, lw in zip(want, low)) and want[1][r.span] == 0


@pytest.mark.parametrize("placement", _far.WRAPS, ids=_far.pid)
def test_parse_wraps_discriminate(placement):
    r = _far.parse_batch(placement, MIX)
    want, low = _far.parse_model(r), _far.parse_model(r, low=True)
    assert want["status"][r.span] == 0 and low["status"][r.span] == (2 if placement[0] == "wrap_frame" else 1)
    assert want["data_off"][r.span] != low["data_off"][r.span] and low["data_off"][r.span] == 0
    if placement[0] == "wrap_frame":
        assert want["n_options"][r.span] == 4 and want["offset"][r.span] == 10
    # and behind the span the device's data_off is the twin's plus D wherever a segment parsed
    ok = want["status"][r.span + 1:] == 0
    assert ok.sum() > 100
    assert (want["data_off"][r.span + 1:][ok] >= np.uint64(_far.TWO32)).all()
    assert (want["data_off"][r.span + 1:][~ok] == 0).all()


@pytest.mark.parametrize("flow", [False, True], ids=["gro", "gro_flow"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_wrap_frame_discriminates(ipver, flow):
    r, valid = _far.gro_batch(ipver, ("wrap_frame", 0), MIX, flow)
    want = _far.gro_model(ipver, r.buf, r.offs, valid, flow)
    low = _far.gro_model(ipver, r.low_buf, r.low_offs, valid, flow)
    sp = r.span
    assert want["frame_seg"][sp] == _gro.NONE and low["frame_seg"][sp] != _gro.NONE  # the span is no member
    # the near run and the far run are one super-segment through f on the low-32 twin, two on the twin
    assert low["frame_seg"][sp - 1] == low["frame_seg"][sp] == low["frame_seg"][sp + 1]
    assert want["frame_seg"][sp - 1] != want["frame_seg"][sp + 1]
    assert want["n_super"] == low["n_super"] + 1
    s_near, s_far = want["frame_seg"][sp - 1], want["frame_seg"][sp + 1]
    assert want["frame_cnt"][s_near] == _far.BRIDGE_NEAR and want["frame_cnt"][s_far] == _far.BRIDGE_FAR
    assert low["frame_cnt"][low["frame_seg"][sp]] == _far.BRIDGE_NEAR + 1 + _far.BRIDGE_FAR


@pytest.mark.parametrize("flow", [False, True], ids=["gro", "gro_flow"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_wrap_empty_has_nothing_to_tell_and_straddle_run_is_merged(ipver, flow):
    r, valid = _far.gro_batch(ipver, ("wrap_empty", 0), MIX, flow)
    want = _far.gro_model(ipver, r.buf, r.offs, valid, flow)
    low = _far.gro_model(ipver, r.low_buf, r.low_offs, valid, flow)
    assert all(np.array_equal(want[k], low[k]) for k in want) and want["frame_seg"][r.span] == _gro.NONE
    for a in range(4):
        r, valid = _far.gro_batch(ipver, ("straddle", a), MIX, flow)
        want = _far.gro_model(ipver, r.buf, r.offs, valid, flow)
        x = _far.crossing(r.far_offs)[0]
        assert want["frame_cnt"][want["frame_seg"][x]] == _far.BRIDGE_FAR  # the frame across byte 2^32 is in a merged run


@pytest.mark.parametrize("ipver", [4, 6])
def test_nat_wraps(ipver):
    for placement in _far.WRAPS:
        r, valid, table, slots, dec = _far.nat_batch(ipver, placement, MIX)
        want, hit = _far.nat_model(ipver, r.buf, r.offs, valid, table, slots, dec)
        low, low_hit = _far.nat_model(ipver, r.low_buf, r.low_offs, valid, table, slots, dec)
        s0 = int(r.offs[r.span])
        assert not hit[r.span] and np.array_equal(want[s0:s0 + r.S_twin], r.buf[s0:s0 + r.S_twin])
        keep = np.arange(r.n) != r.span
        assert np.array_equal(hit[keep], low_hit[keep]) and 100 < hit.sum() < 500
        if placement[0] == "wrap_frame":  # rewritten bytes and the hit bit
            n = r.S % _far.TWO32
            assert low_hit[r.span] and not np.array_equal(low[s0:s0 + n], r.buf[s0:s0 + n])
        else:  # an empty frame is not translated either
            assert not low_hit[r.span]
            assert np.array_equal(np.delete(want, np.s_[s0:s0 + r.S_twin]), low)
