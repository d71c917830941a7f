"""Flow-keyed receive coalescing on the GPU (nsx_gro_flow_ipv4_tcp_dev / nsx_gro_flow_ipv6_tcp_dev): every output
array, d_order included, against the numpy restatement tests/_gro_flow.py (held to tests/_gro.py and to segmentation
offload's expansion by tests/test_gro_flow_abi.py), over outputs pre-filled with a fill byte so that the untouched
regions are compared too. Bit-exact throughout."""
import functools

import numpy as np
import pytest

import _gro
import _gro_flow as FL
import _gro_gpu as G
import _tx
from _gpu import host, setup_gpu, torch, nsx

pytestmark = pytest.mark.gpu

F = _gro
FILL = G.FILL
MSS_OPT = b"\x02\x04\x05\xb4"
SMALL_TILES = dict(rows=1, run_segs=16)  # 256 keys per sort tile, 16 frames per scan block
_d, _d_valid, _same = G.d, G.d_valid, G.same


def setup_module(module):
    setup_gpu()


def _fn(ipver, flow=True):
    return G.fn(ipver, flow)


def _filled(n, ipver, nbytes, flow=True):
    return G.filled(n, ipver, nbytes, flow)


def _host(res, n, ipver, nbytes, flow=True):
    return G.to_host(res, n, ipver, nbytes, flow)


def _gpu(buf, offs, valid, ipver, tune=None, d_valid=None, flow=True):
    return G.gpu(buf, offs, valid, ipver, tune=tune, d_mask=d_valid, flow=flow)


def _want(buf, offs, valid, ipver, flow=True):
    return G.want(buf, offs, valid, ipver, flow)


def _check(buf, offs, valid, ipver, tunes=(None,), what=""):
    return G.check(buf, offs, valid, ipver, tunes=tunes, what=what, flow=True)


# ---------------------------------------------------------------- interleave
@pytest.mark.parametrize("opt", [False, True], ids=["noopt", "opt"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_five_interleaved_connections(ipver, opt):
    """5 connections x 4 frames (700, 700, 700, 300) round-robin, one frame's valid bit clear, behind 0-3 lead bytes:
    6 super-segments where coalescing by adjacency gives 19."""
    for lead in range(4):
        buf, offs, valid = FL.five_by_four(ipver, opt=MSS_OPT if opt else b"", lead=lead)
        o = _check(buf, offs, valid, ipver, tunes=(None, SMALL_TILES), what=f"lead={lead}")
        assert o["n_super"] == 6 and o["order"][-1] == FL.INVALID
    assert _gpu(buf, offs, valid, ipver, flow=False)["n_super"][0] == 19


# ---------------------------------------------------------------- the sort at tile edges
@functools.lru_cache(maxsize=None)
def _interleaved(ipver, n=700, conns=37):
    """n frames of `conns` connections in a seeded random interleave, payloads of 1-4 bytes; a prefix of it is an
    interleave too."""
    rng = np.random.default_rng(0x5F8 + ipver)
    who = rng.integers(0, conns, n)
    cnt = np.bincount(who, minlength=conns)
    flows = FL.connections(rng, ipver, [rng.integers(1, 5, max(int(c), 1)) for c in cnt])
    nxt = [0] * conns
    frames = []
    for c in who:
        frames.append(flows[c][nxt[c]])
        nxt[c] += 1
    return tuple(frames)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 513, 700])
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_sort_at_tile_edges(ipver, n):
    """37 connections in a random interleave, n at and around the 256-key tile of rows = 1 (several tiles, the last
    one partial or exactly full) and inside one default tile: 37 random keys make every digit pass permute, and the
    ~19 equal keys of a connection come out in arrival order only if the rank inside a tile is stable."""
    buf, offs = F.pack(list(_interleaved(ipver)[:n]), lead=n % 4)
    valid = np.ones(n, bool)
    o = _check(buf, offs, valid, ipver, tunes=(SMALL_TILES, None, dict(rows=2)), what=f"n={n}")
    keys = FL.keys(buf, offs, valid, ipver)
    assert np.unique(keys).size == min(n, 37) or n < 255
    assert np.array_equal(o["order"], np.argsort(keys, kind="stable"))
    if n >= 255:
        assert o["n_super"] < F.gro(buf, offs, valid, ipver)["n_super"]


@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_table_scan_takes_more_than_one_sweep(ipver):
    """8,500 frames at rows = 1 are 34 tiles: a digit table of 8,704 counters, more than the 8,192 the scan's one
    workgroup takes per sweep, so the carry from the first sweep is in every position of the highest digits, and most
    threads of the second sweep have no counters left. rows = 64 (and anything larger) puts the same frames into
    one tile."""
    n = 8500
    buf, offs = F.pack(list(_interleaved(ipver, n=n, conns=61)), lead=1)
    valid = np.ones(n, bool)
    valid[::97] = False
    _check(buf, offs, valid, ipver, tunes=(SMALL_TILES, dict(rows=64), dict(rows=1000)))
    assert np.unique(FL.keys(buf, offs, valid, ipver)).size == 62


# ---------------------------------------------------------------- the sort's key distributions
def _keyed(frames, ipver, key):
    """The frames moved to the connection whose flow key is `key` (ports crafted, checksums re-fixed)."""
    return [FL.with_ports(f, ipver, FL.ports_for_key(FL.state(f, ipver), key)) for f in frames]


def _interleave(rng, conns):
    """A random interleave of the connections' frames, each connection's own frames in order."""
    who = rng.permutation(np.repeat(np.arange(len(conns)), [len(c) for c in conns]))
    nxt = [0] * len(conns)
    frames = []
    for w in who:
        frames.append(conns[w][nxt[w]])
        nxt[w] += 1
    return frames


@functools.lru_cache(maxsize=None)
def _key_distribution(ipver, dist):
    """(frames, valid, the keys the frames were made for - None where the frame is no member)."""
    rng = np.random.default_rng(0x610 + ipver)
    if dist == "one_connection":  # 700 frames of one key: every wave step of every pass has 64 equal digits
        frames = F.case_frames(F.flow_case(rng, ipver, [4] * 700))
        return tuple(frames), np.ones(700, bool), None
    if dist == "descending":  # 700 one-frame connections, keys strictly falling: the order is the exact reverse
        keys = np.sort(rng.choice(0xFFFFFFFF, 700, replace=False))[::-1]
        base = F.case_frames(F.flow_case(rng, ipver, [4] * 700))
        frames = [_keyed([f], ipver, int(k))[0] for f, k in zip(base, keys)]
        return tuple(frames), np.ones(700, bool), keys
    if dist.startswith("byte"):  # all 256 values in one key byte, the other three constant; every key three times
        shift = 8 * int(dist[4])
        const = int(rng.integers(1 << 32)) & ~(0xFF << shift) & 0xFFFFFFFF
        if shift == 24:
            const &= ~1  # 0xFFFFFFFF stays the non-members' key alone
        conns = FL.connections(rng, ipver, [(4, 4, 4)] * 256)
        conns = [_keyed(c, ipver, const | (int(j) << shift)) for j, c in zip(rng.permutation(256), conns)]
        return tuple(_interleave(rng, conns)), np.ones(768, bool), None
    assert dist == "extremes"  # keys 0 and 0xFFFFFFFE alternate, every fifth frame a non-member (0xFFFFFFFF)
    a, b = FL.connections(rng, ipver, [[4] * 300, [4] * 300])
    a, b = _keyed(a, ipver, 0), _keyed(b, ipver, 0xFFFFFFFE)
    frames, valid = [], []
    for i in range(300):
        frames += [a[i], b[i]]
        valid += [True, True]
        if i % 2 == 0:  # a truncated frame, or a whole one whose valid bit is clear
            frames.append(a[i][:30] if i % 4 == 0 else b[i])
            valid.append(i % 4 == 0)
    return tuple(frames), np.array(valid), None


KEY_DISTS = ("one_connection", "descending", "byte0", "byte1", "byte2", "byte3", "extremes")


@pytest.mark.parametrize("dist", KEY_DISTS)
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_sort_key_distributions(ipver, dist):
    """Keys crafted through the ports, 700-768 frames (three tiles at rows = 1, one by default). One connection: 64
    equal digits in every wave step, the order the identity across waves and tiles. Strictly descending keys: the
    exact reverse. All 256 values in one key byte and the others constant: that pass permutes with every digit in use
    (64 different digits in a wave step) while the other three must keep the order. Keys 0 and 0xFFFFFFFE alternating
    among non-members: the extreme digits in every pass. The order against a stable argsort of the keys, and every
    output against the model."""
    frames, valid, made = _key_distribution(ipver, dist)
    n = len(frames)
    assert 600 <= n <= 1100
    buf, offs = F.pack(list(frames), lead=n % 4)
    o = _check(buf, offs, valid, ipver, tunes=(dict(rows=1), None), what=dist)
    keys = FL.keys(buf, offs, valid, ipver)
    assert np.array_equal(o["order"], np.argsort(keys, kind="stable"))
    if dist == "one_connection":
        assert np.unique(keys).size == 1 and o["order"].tolist() == list(range(n)) and o["frame_cnt"].tolist() == [n]
    elif dist == "descending":
        assert np.array_equal(keys, made) and (np.diff(keys.astype(np.int64)) < 0).all()
        assert o["order"].tolist() == list(range(n))[::-1] and o["n_super"] == n
    elif dist.startswith("byte"):
        shift = 8 * int(dist[4])
        assert np.unique(keys).size == 256 and np.unique(keys >> shift & 0xFF).size == 256
        assert np.unique(keys & ~np.uint32(0xFF << shift)).size == 1
        assert o["n_super"] == 256 and (o["frame_cnt"] == 3).all()
    else:
        assert set(keys.tolist()) == {0, 0xFFFFFFFE, 0xFFFFFFFF} and o["frame_cnt"].tolist() == [300, 300]
        assert o["order"][:300].tolist() == [i for i in range(n) if keys[i] == 0]


# ---------------------------------------------------------------- the emit grid's second trip
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_emit_grid_takes_a_second_trip(ipver):
    """The batch of test_gpu_gro.py's test of that name (64 x CUs + 21 frames, four connections whose every seventh
    frame ends a run, every 997th valid bit clear) delivered round-robin, at blocks_per_cu = 1: the ordered emit
    pass goes round its grid-stride loop again, once behind one sort tile per 4,096 keys and once behind one per 256."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 21
    assert n > 64 * cus and (n + 15) // 16 > 4 * cus
    frames, _ = FL.round_robin(F.cycle_connections(ipver, n))
    buf, offs = F.pack(frames, lead=ipver % 4)
    assert offs.size - 1 == n
    valid = np.ones(n, bool)
    valid[996::997] = False
    o = _check(buf, offs, valid, ipver, tunes=(dict(blocks_per_cu=1), dict(blocks_per_cu=1, rows=1)))
    assert n // 7 <= o["n_super"] <= n // 7 + 4 + 2 * (n // 997 + 1) and o["frame_cnt"].max() == 7
    assert np.unique(FL.keys(buf, offs, valid, ipver)).size == 5


# ---------------------------------------------------------------- collisions
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_key_collision_never_merges_across_connections(ipver):
    """Two different connections forced to one key, interleaved frame by frame: they stay interleaved (equal keys keep
    arrival order), same() keeps them apart, nothing merges."""
    rng = np.random.default_rng(0x5FA + ipver)
    a, b = FL.connections(rng, ipver, [(700, 700, 700), (700, 700, 700)])
    ports = FL.colliding_ports(a[0], b[0], ipver)
    b = [FL.with_ports(f, ipver, ports) for f in b]
    frames, _ = FL.round_robin([a, b])
    buf, offs = F.pack(frames, lead=2)
    valid = np.ones(6, bool)
    assert np.unique(FL.keys(buf, offs, valid, ipver)).size == 1
    o = _check(buf, offs, valid, ipver, tunes=(None, SMALL_TILES))
    assert o["order"].tolist() == list(range(6)) and o["n_super"] == 6
    # each alone coalesces: the collision is what costs the merges
    assert F.gro(*F.pack(b), np.ones(3, bool), ipver)["n_super"] == 1


@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_member_with_the_non_members_key(ipver):
    """A connection whose key is 0xFFFFFFFF sorts among the non-members, in arrival order: a non-member between two of
    its frames breaks the run, its other frames still merge."""
    rng = np.random.default_rng(0x5FC + ipver)
    a, b = FL.connections(rng, ipver, [(700, 700, 700, 700), (700, 700)])
    ports = FL.ports_for_key(FL.state(a[0], ipver), 0xFFFFFFFF)
    a = [FL.with_ports(f, ipver, ports) for f in a]
    frames = [a[0], b[0], a[1], b[1], b[1], a[2], a[3]]  # frame 4: a duplicate whose valid bit is clear
    valid = np.ones(7, bool)
    valid[4] = False
    buf, offs = F.pack(frames, lead=1)
    assert FL.keys(buf, offs, valid, ipver)[[0, 2, 4, 5, 6]].tolist() == [0xFFFFFFFF] * 5
    o = _check(buf, offs, valid, ipver, tunes=(None, SMALL_TILES))
    assert o["order"].tolist() == [1, 3, 0, 2, 4, 5, 6] and o["frame_cnt"].tolist() == [2, 2, 2]
    assert o["frame_seg"].tolist() == [1, 0, 1, 0, F.NONE, 2, 2]


# ---------------------------------------------------------------- non-members
def _non_member_batch(ipver):
    """Three connections round-robin (4 frames each); frames 1, 4, 6 and 9 made non-members with the valid bit still
    set: a total / payload length one short of the frame, doff 4, doff past the segment, a truncated frame."""
    rng = np.random.default_rng(0x5FE + ipver)
    frames, _ = FL.round_robin(FL.connections(rng, ipver, [(30, 30, 30, 30)] * 3))
    tcp = 20 if ipver == 4 else 40
    at = 2 if ipver == 4 else 4

    def length(fr):
        fr[at:at + 2] = (int.from_bytes(fr[at:at + 2], "big") - 1).to_bytes(2, "big")

    def doff(v):
        return lambda fr: fr.__setitem__(tcp + 12, v)

    for i, change in ((1, length), (4, doff(0x40)), (6, doff(0xF0))):
        fr = bytearray(frames[i])
        change(fr)
        frames[i] = F.refix(fr, ipver)
    frames[9] = frames[9][:tcp + 10]
    return frames, [1, 4, 6, 9]


@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_non_members_come_last_in_arrival_order(ipver):
    frames, bad = _non_member_batch(ipver)
    buf, offs = F.pack(frames, lead=3)
    valid = np.ones(12, bool)
    valid[[3, 11]] = False  # and two clear valid bits
    o = _check(buf, offs, valid, ipver, tunes=(None, SMALL_TILES))
    out = sorted(bad + [3, 11])
    assert o["order"][-6:].tolist() == out and (o["frame_seg"][out] == F.NONE).all()
    assert (o["frame_seg"][[i for i in range(12) if i not in out]] != F.NONE).all()


@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_with_the_receive_pass_mask(ipver):
    """d_valid straight from nsx_rx_*_tcp_verify_dev over the same batch, one frame's TCP checksum corrupted: that
    frame is the one the mask drops, and it comes last."""
    frames, bad = _non_member_batch(ipver)
    tcp = 20 if ipver == 4 else 40
    fr = bytearray(frames[7])
    fr[tcp + 16] ^= 0x55
    frames[7] = bytes(fr)
    buf, offs = F.pack(frames)
    rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    d_mask = rx(_d(buf), _d(offs))
    valid = host(d_mask).view(np.uint64)
    bits = F.valid_bits(valid, 12)
    assert not bits[7] and bits[[0, 2, 3, 5, 8, 10, 11]].all()
    want, o = _want(buf, offs, valid, ipver)
    _same(_gpu(buf, offs, valid, ipver, d_valid=d_mask), want)
    assert o["order"][-5:].tolist() == sorted(bad + [7])


# ---------------------------------------------------------------- round trip on the device
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_round_trip_on_the_device(ipver):
    """flow GRO → nsx_tso_*_build_dev without leaving the device: output position p is input frame order[p], byte for
    byte, for every member (4-multiple frame lengths, so the build's slots are packed)."""
    buf, offs, valid = FL.five_by_four(ipver, opt=MSS_OPT)
    n = offs.size - 1
    g = _fn(ipver)(_d(buf), _d(offs), _d_valid(valid, n))
    ns = int(g["n_super"].item())
    assert ns == 6
    order = g["order"].to(torch.int64)
    nf = int(g["frame_cnt"][:ns].sum().item())
    assert nf == 19
    d_offs = _d(offs)
    flen = (d_offs[1:] - d_offs[:-1])[order[:nf]]
    assert not bool((flen % 4).any())
    out_off = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    out_off[1:] = torch.cumsum(flen, 0)
    frame_first = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    frame_first[1:] = torch.cumsum(g["frame_cnt"][:ns].to(torch.int64), 0)
    assert torch.equal(frame_first[:ns], g["first_frame"][:ns])  # positions: members first, so the prefix sum
    seg = g["frame_seg"][order[:nf]].contiguous()  # frame_seg of position p
    alen = 4 if ipver == 4 else 16
    built = torch.full((int(out_off[-1].item()),), FILL, dtype=torch.uint8, device="cuda")
    tso = nsx.tso_ipv4_tcp_build_dev if ipver == 4 else nsx.tso_ipv6_tcp_build_dev
    tso({k: g[k][:ns * (alen if k in ("src", "dst") else 1)] for k in nsx.IP_FIELDS},
        {k: g[k][:ns] for k, _ in nsx.BUILD_FIELDS}, g["data"], g["data_off"][:ns + 1], g["mss"][:ns], frame_first, seg,
        built, out_off, opts=g["opts"], opt_off=g["opt_off"][:ns + 1])
    z, oo, od = host(built), host(out_off), host(order)
    for p in range(nf):
        f = int(od[p])
        assert z[int(oo[p]):int(oo[p + 1])].tobytes() == buf[int(offs[f]):int(offs[f + 1])].tobytes(), (p, f)


# ---------------------------------------------------------------- tiny batches
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_empty_batch_and_one_frame(ipver):
    """n == 0 writes n_super = 0 and the two leading offsets and leaves d_order alone; n == 1 is one super-segment
    (or none, with the valid bit clear)."""
    buf, offs = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    want, _ = _want(buf, offs, np.zeros(0, bool), ipver)
    assert want["n_super"][0] == 0 and want["opt_off"][0] == 0 and want["data_off"][0] == 0
    assert (want["order"].view(np.uint8) == FILL).all()
    _same(_gpu(buf, offs, np.zeros(0, bool), ipver), want)
    rng = np.random.default_rng(0x600 + ipver)
    buf, offs = F.pack(F.case_frames(F.flow_case(rng, ipver, [9])), lead=1)
    for v, ns in ((True, 1), (False, 0)):
        o = _check(buf, offs, np.array([v]), ipver, tunes=(None, SMALL_TILES))
        assert o["n_super"] == ns and o["order"].tolist() == [0]


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("ipver", [4, 6])
def test_flow_device_call_captures_into_a_graph(ipver):
    """No allocation, no host sync: one call captured on a side stream (a single chain of launches), replayed twice
    into re-filled outputs, gives the model's arrays both times."""
    buf, offs = F.pack(list(_interleaved(ipver)[:300]), lead=1)
    n = 300
    valid = np.ones(n, bool)
    valid[[5, 77]] = False
    want, _ = _want(buf, offs, valid, ipver)
    d_buf, d_offs, d_valid = _d(buf), _d(offs), _d_valid(valid, n)
    fn = _fn(ipver)
    fn(d_buf, d_offs, d_valid, tune=SMALL_TILES)  # a first call outside capture (library and device-info setup)
    torch.cuda.synchronize()
    out = _filled(n, ipver, buf.size)
    order = out.pop("order")
    work = torch.empty(nsx.gro_flow_work_bytes(n), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(d_buf, d_offs, d_valid, out=out, order=order, work=work, tune=SMALL_TILES)
    torch.cuda.synchronize()
    assert (host(order).view(np.uint8) == FILL).all() and (host(out["frame_seg"]).view(np.uint8) == FILL).all()
    for _ in range(2):
        g.replay()
        _same(_host(dict(out, order=order), n, ipver, buf.size), want, "replay")
        for t in list(out.values()) + [order, work]:
            t.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()


# ---------------------------------------------------------------- existing behaviour
@pytest.mark.parametrize("ipver", [4, 6])
def test_adjacency_call_is_unchanged_on_an_interleaved_batch(ipver):
    """nsx_gro_* over the interleaved batches above still equals tests/_gro.gro, array for array."""
    for buf, offs, valid in (FL.five_by_four(ipver, opt=MSS_OPT, lead=1),
                             F.pack(list(_interleaved(ipver)[:300]), lead=2) + (np.ones(300, bool),)):
        want, _ = _want(buf, offs, valid, ipver, flow=False)
        for tune in (None, dict(run_segs=16), SMALL_TILES):
            _same(_gpu(buf, offs, valid, ipver, tune=tune, flow=False), want, f"tune={tune}")
