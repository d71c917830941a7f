"""Flow-keyed receive coalescing (nsx_gro_flow_ipv4_tcp_dev / nsx_gro_flow_ipv6_tcp_dev) restated in numpy and plain
Python, without looking at the library: the flow key of include/nsx_csum.h, the stable order, and the outputs as
tests/_gro.py gives them over the frames repacked in that order. tests/test_gro_flow_abi.py holds it to what already
exists: tests/_gro.py on a single connection, segmentation offload's expansion (tests/_tso.py) on interleaved ones."""
import numpy as np

import _gro

NO_FLOW = 0xFFFFFFFF
FNV_BASIS, FNV_PRIME, M32 = 0x811C9DC5, 0x01000193, 0xFFFFFFFF
FNV_PRIME_INV = pow(FNV_PRIME, -1, 1 << 32)


def _dwords(frame: bytes, ipver: int):
    """The dwords the key is made of, little-endian, in order: the addresses, then the ports (a member's frame)."""
    ihl = (frame[0] & 15) * 4 if ipver == 4 else 40
    a = frame[12:20] if ipver == 4 else frame[8:40]
    return [int.from_bytes(a[k:k + 4], "little") for k in range(0, len(a), 4)] + \
        [int.from_bytes(frame[ihl:ihl + 4], "little")]


def _mix(h: int, w: int) -> int:
    return ((h ^ w) * FNV_PRIME) & M32


def state(frame: bytes, ipver: int) -> int:
    """The hash of a member's frame before its last dword, the ports, goes in."""
    h = FNV_BASIS
    for w in _dwords(frame, ipver)[:-1]:
        h = _mix(h, w)
    return h


def key(frame: bytes, ipver: int) -> int:
    """The flow key of a frame whose valid bit is set: 0xFFFFFFFF unless it is a member (tests/_gro.parse)."""
    if _gro.parse(frame, ipver) is None:
        return NO_FLOW
    return _mix(state(frame, ipver), _dwords(frame, ipver)[-1])


def keys(buf, offsets, valid, ipver: int):
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    ok = _gro.valid_bits(valid, n)
    return np.array([key(buf[int(offsets[i]):int(offsets[i + 1])].tobytes(), ipver) if ok[i] else NO_FLOW
                     for i in range(n)], np.uint32).reshape(n)


def order(buf, offsets, valid, ipver: int):
    """The stable ascending sort of the frame indices by key (uint32)."""
    return np.argsort(keys(buf, offsets, valid, ipver), kind="stable").astype(np.uint32)


def gro_flow(buf, offsets, valid, ipver: int) -> dict:
    """The outputs of the device call: tests/_gro.gro over the frames repacked in key order (first_frame holds
    positions in that order), frame_seg turned back to the original frame indices, plus `order`."""
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    ok = _gro.valid_bits(valid, n)
    od = order(buf, offsets, valid, ipver)
    frames = [buf[int(offsets[f]):int(offsets[f + 1])].tobytes() for f in od]
    buf2, offs2 = _gro.pack(frames)
    out = _gro.gro(buf2, offs2, ok[od], ipver)
    seg = np.full(n, _gro.NONE, np.uint32)
    seg[od] = out["frame_seg"]
    out["frame_seg"] = seg
    out["order"] = od
    return out


def colliding_ports(a: bytes, b: bytes, ipver: int) -> int:
    """The ports dword (little-endian TCP bytes 0-3) that gives connection b (one of its frames) the key of connection
    a: p_b = p_a ^ state_a ^ state_b — the last step (h ^ w) * prime is a bijection in w."""
    return ports_of(a, ipver) ^ state(a, ipver) ^ state(b, ipver)


def ports_for_key(st: int, k: int) -> int:
    """The ports dword that gives a connection with state st the key k."""
    return ((k * FNV_PRIME_INV) & M32) ^ st


def with_ports(frame: bytes, ipver: int, ports: int) -> bytes:
    """The frame with its TCP bytes 0-3 replaced by the dword `ports` (little-endian), checksums re-fixed."""
    f = bytearray(frame)
    ihl = (f[0] & 15) * 4 if ipver == 4 else 40
    f[ihl:ihl + 4] = int(ports).to_bytes(4, "little")
    return _gro.refix(f, ipver)


def ports_of(frame: bytes, ipver: int) -> int:
    return _dwords(frame, ipver)[-1]


def connections(rng, ipver: int, pays_per_conn, opt: bytes = b""):
    """One list of frames per connection (tests/_gro.flow_case each): different addresses, ports and sequence
    numbers, frames of one connection in order."""
    return [_gro.case_frames(_gro.flow_case(rng, ipver, pays, opt=opt)) for pays in pays_per_conn]


def round_robin(conns):
    """Frame 0 of every connection, then frame 1 of every connection, ...: (frames, connection of each frame)."""
    frames, who = [], []
    for j in range(max(len(c) for c in conns)):
        for ci, c in enumerate(conns):
            if j < len(c):
                frames.append(c[j])
                who.append(ci)
    return frames, who


INVALID = 7  # five_by_four: frame 1 of connection 2


def five_by_four(ipver: int, opt: bytes = b"", lead: int = 0):
    """5 connections of 4 frames (payloads 700, 700, 700, 300) delivered round-robin, the valid bit of frame INVALID
    (the second frame of connection 2) clear: (buf, offsets, valid). By adjacency every valid frame is its own
    super-segment, 19; per connection four connections give one each and connection 2 gives [700] and [700, 300]: 6."""
    rng = np.random.default_rng(0x5F4 + ipver)
    frames, _ = round_robin(connections(rng, ipver, [(700, 700, 700, 300)] * 5, opt=opt))
    buf, offs = _gro.pack(frames, lead=lead)
    valid = np.ones(len(frames), bool)
    valid[INVALID] = False
    return buf, offs, valid
