"""UDP receive coalescing on the GPU (nsx_ugro_ipv4_dev / nsx_ugro_ipv6_dev and the flow-keyed nsx_ugro_flow_*): every
case compares the kernels with the numpy restatement tests/_ugro.py — every output array and the regions that must stay
untouched (the outputs are pre-filled with a fill byte) — for both IP versions and both forms, at the smallest shapes at
which each pass can go wrong; then the round trip through the UDP receive verify and UDP segmentation offload without
the host, graph capture, and a batch that lies past 2^32 in its arena."""
import numpy as np
import pytest

import _far
import _gro_flow as FL
import _udp
import _ugro as UG
import _ugro_gpu as GPU
from _gpu import host, setup_gpu, torch, nsx

pytestmark = pytest.mark.gpu

SMALL = dict(run_segs=16, blocks_per_cu=1, rows=1)
TUNES = (None, SMALL)
ipvers = pytest.mark.parametrize("ipver", [4, 6])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    setup_gpu()


def _rng(*k):
    return np.random.default_rng([0x06C0, *k])


# ---------------------------------------------------------------- head pass
@pytest.mark.parametrize("n", [62, 63, 64, 126, 127])
@ipvers
def test_one_run_across_the_head_pass_wave_boundary(ipver, n):
    """A wave of the head pass owns 63 frames and reads the frame before them in lane 0: one flow of n equal
    datagrams is one super-datagram whatever n is, and a short tail stays with it."""
    rng = _rng(1, ipver, n)
    buf, offs = UG.pack(UG.flow_frames(rng, ipver, [24] * (n - 1) + [5]), lead=n % 4)
    o, _ = GPU.check_both(buf, offs, np.ones(n, bool), ipver, TUNES, f"n={n}")
    assert o["n_super"] == 1 and o["frame_cnt"][0] == n


@pytest.mark.parametrize("k", [62, 63, 64])
@ipvers
def test_a_run_ends_and_starts_at_the_wave_boundary(ipver, k):
    """127 frames: a flow of k datagrams, then another flow — the run ends one frame before, exactly at, and one frame
    behind the boundary between the first wave's frames (0..62) and the second's."""
    rng = _rng(2, ipver, k)
    frames = UG.flow_frames(rng, ipver, [9] * k) + UG.flow_frames(rng, ipver, [9] * (127 - k))
    buf, offs = UG.pack(frames, lead=1)
    o, _ = GPU.check_both(buf, offs, np.ones(127, bool), ipver, TUNES, f"k={k}")
    assert o["frame_cnt"].tolist() == [k, 127 - k]


# ---------------------------------------------------------------- scan
@ipvers
def test_runs_straddle_scan_block_edges(ipver):
    """run_segs=16: 330 frames span 21 scan blocks. Runs of 1, 15, 16, 17, 31, 32, 33 and 5 frames in turn put heads,
    tails and whole runs on either side of the block edges; the three-frame window is read across an edge too."""
    rng = _rng(3, ipver)
    frames, runs = [], []
    while len(frames) < 330:
        k = (1, 15, 16, 17, 31, 32, 33, 5)[len(runs) % 8]
        g = int(rng.integers(2, 40))
        frames += UG.flow_frames(rng, ipver, [g] * (k - 1) + [int(rng.integers(1, g + 1))])
        runs.append(k)
    frames = frames[:330]
    buf, offs = UG.pack(frames, lead=2)
    o, _ = GPU.check_both(buf, offs, np.ones(330, bool), ipver, TUNES)
    assert o["frame_cnt"].tolist()[:8] == [1, 15, 16, 17, 31, 32, 33, 5]
    # strictly decreasing payloads over a block edge: frames 14..18 of one flow
    frames = UG.flow_frames(rng, ipver, [60] * 14 + [50, 40, 30, 20, 10] + [10] * 20)
    buf, offs = UG.pack(frames)
    o, _ = GPU.check_both(buf, offs, np.ones(len(frames), bool), ipver, TUNES)
    assert o["frame_cnt"].tolist() == [15, 1, 1, 1, 1, 20]


# ---------------------------------------------------------------- emit pass
SMALL_PAYS = tuple(range(1, 18)) + (31, 32, 33)


def _aligned_pays(lengths):
    """Payload lengths of one flow in which every length of `lengths` starts at every destination alignment 0..15:
    before each a filler of 1..16 bytes brings the packed payload offset to the alignment wanted."""
    pays, at = [], 0
    for L in lengths:
        for a in range(16):
            fill = (a - at) % 16 or 16
            pays += [fill, L]
            at += fill + L
    return pays


@pytest.mark.parametrize("leads", [range(0, 4), range(4, 8), range(8, 12), range(12, 16)], ids=lambda r: f"lead{r[0]}")
@ipvers
def test_short_payloads_at_every_source_and_destination_alignment(ipver, leads):
    """Payloads of 1..17 and 31..33 bytes, each at every destination alignment 0..15 (the fillers before them), the
    batch behind 0..15 lead bytes — every source alignment against every destination alignment. All frames are of one
    flow with counting idents, so a payload that is no longer than the one before it joins it: two payloads meet
    inside one dword, and a head's payload starts where the last run's ended."""
    pays = _aligned_pays(SMALL_PAYS)
    for lead in leads:
        rng = _rng(4, ipver, lead)
        c = UG.flow_case(rng, ipver, pays)
        frames = UG.case_frames(c)
        buf, offs = UG.pack(frames, lead=lead)
        GPU.check(buf, offs, np.ones(len(pays), bool), ipver, TUNES if lead == leads[0] else (None,), f"lead={lead}")
    GPU.check(buf, offs, np.ones(len(pays), bool), ipver, (SMALL,), flow=True)


@ipvers
def test_long_payloads_cross_the_copy_row_at_every_alignment(ipver):
    """8972-byte payloads (five row pairs of the copy, 2 KiB of destination each) at every destination alignment, behind
    0..15 lead bytes; 1472 bytes; and the longest datagram the IP version can carry."""
    big = _udp.PAY_MAX[ipver]
    pays = _aligned_pays((8972,)) + [1472, 1472, 100, big]
    for lead in range(16):
        rng = _rng(5, ipver, lead)
        buf, offs = UG.pack(UG.flow_frames(rng, ipver, pays), lead=lead)
        o = GPU.check(buf, offs, np.ones(len(pays), bool), ipver, (None,), f"lead={lead}", flow=lead % 2 == 1)
        assert o["gso"][-1] == big and o["frame_cnt"][-3:].tolist() == [2, 2, 1]
    rng = _rng(5, ipver, 99)
    pays = [big, big, big, 8972]
    buf, offs = UG.pack(UG.flow_frames(rng, ipver, pays), lead=3)
    o, _ = GPU.check_both(buf, offs, np.ones(4, bool), ipver, TUNES)
    assert o["n_super"] == 1 and int(o["data_off"][1]) == sum(pays) > 1 << 17  # no 64 KiB cap on a super-datagram
    GPU.assert_round_trip(buf, offs, ipver, members=4)


@ipvers
def test_emit_grid_takes_a_second_trip(ipver):
    """blocks_per_cu=1: the emit grid has one block (four wave tasks of 16 frames) per CU, so a batch of more than 64
    frames per CU sends every wave round its loop again. A block of 64 datagrams of one flow (idents 0..63) repeated:
    the run breaks where the ident falls back."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = _rng(6, ipver)
    block = UG.flow_frames(rng, ipver, [6, 6, 6, 3, 16, 16, 1, 33] * 8, ident0=0)
    reps = cus + 2
    n = 64 * reps + 5
    buf, offs = UG.pack((block * (reps + 1))[:n], lead=1)
    o = GPU.check(buf, offs, np.ones(n, bool), ipver, (dict(blocks_per_cu=1), None))
    assert o["frame_cnt"][:4].tolist() == [4, 3, 2, 3]
    GPU.check(buf, offs, np.ones(n, bool), ipver, (dict(blocks_per_cu=1, rows=1),), flow=True)


# ---------------------------------------------------------------- flow form
def _keyed(rng, ipver, keys, per=3, pay=11):
    """One flow of `per` datagrams per key, the ports crafted so that the flow has exactly that key."""
    flows = []
    for k in keys:
        fr = UG.flow_frames(rng, ipver, [pay] * per)
        flows.append([UG.with_ports(f, ipver, FL.ports_for_key(FL.state(f, ipver), int(k))) for f in fr])
        assert {UG.key(f, ipver) for f in flows[-1]} == {int(k)}
    return flows


@pytest.mark.parametrize("dist", ["equal", "distinct", "digit0", "digit1", "digit2", "digit3", "no_flow"])
@ipvers
def test_flow_form_over_several_sort_tiles_and_crafted_keys(ipver, dist):
    """rows=1: 256 keys per sort tile, so 600 frames span three. Key distributions: all equal (colliding flows: the
    order is the arrival order and nothing merges wrongly), all distinct, one radix digit varying with the other three
    fixed, and members whose key is 0xFFFFFFFF among non-members."""
    rng = _rng(7, ipver, len(dist), ord(dist[-1]))
    nfl = 200
    if dist == "equal":
        keys = [0x1234ABCD] * nfl
    elif dist == "distinct":
        keys = rng.integers(0, 0xFFFFFFFF, nfl)
        assert np.unique(keys).size == nfl
    elif dist == "no_flow":
        keys = [0xFFFFFFFF] * 20 + list(rng.integers(0, 0xFFFFFFFF, nfl - 20))
    else:
        sh = 8 * int(dist[-1])
        keys = [(0x5A6B7C8D & ~(0xFF << sh)) | (int(v) << sh) for v in rng.integers(0, 256, nfl)]
    frames, _ = FL.round_robin(_keyed(rng, ipver, keys))
    n = len(frames)
    assert n == 600
    buf, offs = UG.pack(frames, lead=1)
    valid = np.ones(n, bool)
    if dist == "no_flow":
        valid[rng.integers(0, n, 40)] = False
    o = GPU.check(buf, offs, valid, ipver, (dict(rows=1), dict(rows=1, run_segs=16), None), dist, flow=True)
    if dist == "distinct":
        assert o["n_super"] == nfl and (o["frame_cnt"] == 3).all()
    if dist == "equal":
        assert o["order"].tolist() == list(range(n))
    GPU.check(buf, offs, valid, ipver, (None,), dist)  # by adjacency: round-robin merges nothing
    if dist != "no_flow":  # there, members sort among the non-members: the round trip's positions are not the first
        GPU.assert_round_trip(buf, offs, ipver, tune=dict(rows=1), flow=True, keep=valid, members=int(valid.sum()))


# ---------------------------------------------------------------- mask
@ipvers
def test_mask_is_obeyed_and_never_trusted(ipver):
    """A clear bit on frames of garbage (they are not read: any length, 0 and 70000 bytes included); a set bit on
    malformed frames — truncated, padded, zero field, wrong protocol, a UDP length past the frame — the last of them a
    truncated frame that ends the exactly sized buffer; n == 0; a batch with no member at all."""
    rng = _rng(8, ipver)
    good = UG.flow_frames(rng, ipver, [40] * 12)
    junk = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 1, 3, 27, 47, 300, 70000)]
    h = UG.IPH[ipver]
    arr = lambda f: np.frombuffer(f, np.uint8)  # noqa: E731
    bad = [bytes(_udp.corrupt(rng, arr(good[0]), ipver, k)) for k in ("padding", "field_zero", "protocol",
                                                                     "udp_len_long", "udp_len_short", "version")]
    bad += [good[1][:h + 7], good[1][:h], good[1][:3], b""]
    frames, valid = [], []
    for k, f in enumerate(good):
        frames += [f] + ([junk[k]] if k < len(junk) else []) + ([bad[k - 1]] if 1 <= k <= len(bad) else [])
        valid += [True] + ([False] if k < len(junk) else []) + ([True] if 1 <= k <= len(bad) else [])
    frames.append(good[2][:h + 5])  # a set bit on a frame cut inside its UDP header, at the very end
    valid.append(True)
    buf, offs = UG.pack(frames, lead=1, exact=True)
    assert buf.size == int(offs[-1])
    valid = np.array(valid)
    o, _ = GPU.check_both(buf, offs, valid, ipver, TUNES)
    assert o["n_super"] == 12 and (o["frame_seg"] != UG.NONE).sum() == 12
    # all non-members: nothing but n_super, data_off[0] and frame_seg is written
    o, _ = GPU.check_both(buf, offs, np.zeros(len(frames), bool), ipver, TUNES)
    assert o["n_super"] == 0
    sel = [i for i, f in enumerate(frames) if f not in good]
    buf2, offs2 = UG.pack([frames[i] for i in sel], exact=True)
    GPU.check_both(buf2, offs2, np.ones(len(sel), bool), ipver, TUNES)
    # n == 0: *n_super = 0 and data_off[0] = 0, nothing else; d_order untouched
    empty, o0 = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    GPU.check_both(empty, o0, np.zeros(0, bool), ipver, TUNES)


# ---------------------------------------------------------------- round trip without the host
@pytest.mark.parametrize("flow", [False, True], ids=["adjacent", "flow"])
@ipvers
def test_round_trip_through_verify_and_segmentation_offload(ipver, flow):
    """nsx_udp_rx_*_verify_dev → nsx_ugro_* → nsx_udp_uso_*_build_dev rebuilds every member frame byte for byte, the
    UDP checksum included — a frame whose stored field is 0xFFFF because the computed checksum is 0 among them — and
    leaves the frames the verify rejects, a padded datagram and (IPv4) a zero-field datagram out."""
    rng = _rng(9, ipver)
    flows = []
    for k in range(6):
        pays = [int(rng.integers(8, 1473))] * int(rng.integers(2, 9)) + [int(rng.integers(2, 8))]
        c = UG.flow_case(rng, ipver, pays)
        if k % 2 == 0:
            _udp.craft_ffff(c, 1, k)  # even and odd payload offsets
        fr = UG.case_frames(c)
        if k % 2 == 0:
            h = UG.IPH[ipver]
            assert fr[1][h + 6:h + 8] == b"\xff\xff"
        flows.append(fr)
    frames, _ = FL.round_robin(flows) if flow else ([f for fl in flows for f in fl], None)
    arr = lambda f: np.frombuffer(f, np.uint8)  # noqa: E731
    extra = [bytes(_udp.corrupt(rng, arr(flows[0][0]), ipver, k)) for k in ("padding", "payload_byte", "field_zero")]
    frames = frames[:5] + extra + frames[5:]
    buf, offs = UG.pack(frames, lead=3)
    for tune in TUNES:
        ps = GPU.assert_round_trip(buf, offs, ipver, tune=tune, flow=flow, members=len(frames) - 3)
        assert not set(ps.tolist()) & {5, 6, 7}
    valid, _, _ = _udp.rx_expected(ipver, buf, offs)
    o = GPU.check(buf, offs, valid, ipver, TUNES, flow=flow)
    assert o["frame_cnt"].max() >= 3 and (flow or o["n_super"] < len(frames) - 3)


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("flow", [False, True], ids=["adjacent", "flow"])
@ipvers
def test_device_call_captures_into_a_graph(ipver, flow):
    """No allocation, no host sync: one call captured on a side stream (a single chain of launches), replayed twice
    into re-filled outputs, gives the model's arrays both times."""
    rng = _rng(10, ipver)
    flows = [UG.flow_frames(rng, ipver, [30] * 7 + [4]) for _ in range(40)]
    frames, _ = FL.round_robin(flows) if flow else ([f for fl in flows for f in fl], None)
    n = len(frames)
    buf, offs = UG.pack(frames, lead=1)
    valid = np.ones(n, bool)
    valid[[5, 77]] = False
    want, _ = GPU.want(buf, offs, valid, ipver, flow)
    d_buf, d_offs, d_valid = GPU.d(buf), GPU.d(offs), GPU.d_valid(valid, n)
    fn = GPU.fn(ipver, flow)
    fn(d_buf, d_offs, d_valid, tune=SMALL)  # a first call outside capture (library and device-info setup)
    torch.cuda.synchronize()
    out = GPU.filled(n, ipver, buf.size, flow)
    order = out.pop("order", None)
    kw = dict(order=order) if flow else {}
    need = nsx.ugro_flow_work_bytes(n) if flow else nsx.ugro_work_bytes(n)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(d_buf, d_offs, d_valid, out=out, work=work, tune=SMALL, **kw)
    torch.cuda.synchronize()
    assert (host(out["frame_seg"]).view(np.uint8) == GPU.FILL).all()  # capture ran nothing
    for _ in range(2):
        g.replay()
        res = dict(out, order=order) if flow else out
        GPU.same(GPU.to_host(res, n, ipver, buf.size, flow), want, "replay")
        for t in list(out.values()) + [work] + ([order] if flow else []):
            t.view(torch.uint8).fill_(GPU.FILL)
        torch.cuda.synchronize()


# ---------------------------------------------------------------- far offsets
@pytest.fixture(scope="module")
def arenas():
    a = torch.zeros(_far.ARENA, dtype=torch.uint8, device="cuda")
    b = torch.empty(_far.ARENA, dtype=torch.uint8, device="cuda")
    yield a, b
    del a, b
    torch.cuda.empty_cache()


@pytest.mark.parametrize("flow", [False, True], ids=["adjacent", "flow"])
@ipvers
def test_frames_past_two_to_the_32(arenas, ipver, flow):
    """A batch in a 4 GiB arena (tests/_far.layout, a straddle placement): 60 near frames, a span of almost 2^32 bytes
    whose valid bit is set and which is no member, and 200 far frames of which one lies across byte 2^32 inside a
    merged run. Every output array against the model on the compact twin; the data array is given at its worst-case
    extent and nothing past the packed payloads is written."""
    arena, data = arenas
    rng = _rng(11, ipver, int(flow))
    bridge = UG.flow_frames(rng, ipver, [48] * 20)
    mk = lambda k: [f for _ in range(k) for f in UG.flow_frames(rng, ipver, [int(rng.integers(1, 90))] * 4 + [1])]  # noqa: E731
    near, far = mk(11) + bridge[:5], bridge[5:] + mk(37)
    if flow:
        near, far = FL.round_robin([near[i::5] for i in range(5)])[0], FL.round_robin([far[i::8] for i in range(8)])[0]
        far = bridge[5:] + [f for f in far if f not in bridge]  # the frame across byte 2^32 stays inside a run
    head = bytes([0x60 if ipver == 6 else 0x45]) + rng.integers(0, 256, _far.HEAD - 1, dtype=np.uint8).tobytes()
    r = _far.layout(near, head, far, ("straddle", 1), lead=int(rng.integers(4)), rng=rng)
    valid = np.ones(r.n, bool)
    nb = r.buf.size
    w, o = GPU.want(r.buf, r.offs, valid, ipver, flow)
    cross = _far.crossing(r.far_offs)
    assert len(cross) == 1 and o["frame_seg"][r.span] == UG.NONE and o["frame_cnt"][o["frame_seg"][cross[0]]] >= 3
    arena.zero_()
    for dst, b in r.pieces():
        if len(b):
            arena[dst:dst + len(b)].copy_(torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()))
    out = GPU.filled(r.n, ipver, 1, flow)
    order = out.pop("order", None)
    assert nb <= 4 << 20
    data[:8 << 20] = GPU.FILL
    out["data"] = data
    kw = dict(order=order) if flow else {}
    res = GPU.fn(ipver, flow)(arena, GPU.d(r.far_offs), GPU.d_valid(valid, r.n), out=out, **kw)
    got = {k: host(res[k][:nb] if k == "data" else res[k]).view(GPU._NP[dt])
           for k, (dt, _) in GPU.sizes(r.n, ipver, nb, flow).items()}
    GPU.same(got, w, "far")
    assert bool((data[nb:8 << 20] == GPU.FILL).all()), "data bytes written past the twin's extent"
