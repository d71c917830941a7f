"""nsx — Python binding of libnsx_csum.so (include/nsx_csum.h) for tests and bench.

The product is the C ABI + gfx950 kernels in ../csrc; this module is plumbing:
ctypes calls with torch tensors as device buffers. There is no fallback of any
kind: if the library is missing, importing a device call raises, and on a host
without a GPU the device calls return NSX_ENODEV, raised here as NsxError.

Reference interface mirrored (transport/tcp/tcp.go:72-95):
    computeChecksum(ipPseudoHeader []byte) uint16  → csum16(prefix, seg) -> int
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libnsx_csum.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "nsx_csum.h")

NSX_OK, NSX_EIO, NSX_ENOMEM, NSX_ENODEV, NSX_EINVAL = 0, -5, -12, -19, -22
# nsx_tune.kernel (include/nsx_tune.h)
KERNEL_HDR_THREAD, KERNEL_HDR_DENSE, KERNEL_BUILD_PLAIN, KERNEL_BUILD_GENERAL, KERNEL_SCAN_PLAIN = 1, 2, 2, 3, 2


class Tune(ctypes.Structure):
    """include/nsx_tune.h: per-call launch overrides (0 = default). Benchmarks and tests only."""
    _fields_ = [("blocks_per_cu", ctypes.c_int32), ("segs_per_wave", ctypes.c_int32),
                ("block_mode", ctypes.c_int32), ("rows", ctypes.c_int32), ("run_segs", ctypes.c_int32),
                ("xcd_chunk", ctypes.c_int32), ("window_bytes", ctypes.c_int64), ("kernel", ctypes.c_int32),
                ("shards_per_device", ctypes.c_int32), ("deal", ctypes.c_int32),
                ("chunk_bytes", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


TUNE_FIELDS = tuple(f for f, _ in Tune._fields_ if f != "reserved")


def _tune(tune):
    """dict (or Tune, or None) → ctypes pointer argument (None = defaults)."""
    if tune is None or isinstance(tune, Tune):
        return None if tune is None else ctypes.byref(tune)
    bad = set(tune) - set(TUNE_FIELDS)
    if bad:
        raise ValueError(f"unknown nsx_tune field(s): {sorted(bad)}")
    return ctypes.byref(Tune(**{k: int(v) for k, v in tune.items()}))


class NsxError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        super().__init__(f"{what}: {lib().nsx_strerror(code).decode()} ({code})")


_lib = None


def lib() -> ctypes.CDLL:
    """Load the in-tree product library; fail loudly if it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libnsx_csum.so not built at {LIB_PATH}: run `make -C network-stack_amd` "
                              "or __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, u64, u32, i32, u8 = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32,
                                     ctypes.c_int, ctypes.c_uint8)
        sig = {
            "nsx_csum16": [vp, sz, vp, sz, vp],
            "nsx_csum_fixed_dev": [vp, u64, u32, u64, vp, vp, vp],
            "nsx_csum_ragged_dev": [vp, vp, u64, vp, vp, vp],
            "nsx_verify_ragged_dev": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_pseudo_ipv4_partial_dev": [vp, vp, vp, u8, u64, vp, vp],
            "nsx_pseudo_ipv6_partial_dev": [vp, vp, vp, u8, u64, vp, vp],
            "nsx_verify_mask_dev": [vp, u64, vp, vp],
            "nsx_host_cache_release": [],
            "nsx_stream_release": [vp],
            "nsx_deal_sets_in_use": [ctypes.POINTER(u32)],
            "nsx_csum_fixed_host": [vp, u64, u32, u64, vp, vp, i32],
            "nsx_csum_ragged_host": [vp, vp, u64, vp, vp, i32],
            "nsx_alloc_pinned": [sz, ctypes.POINTER(vp)],
            "nsx_free_pinned": [vp],
            "nsx_shard_plan": [vp, u64, i32, vp],
            "nsx_fill_splitmix64_dev": [vp, u64, u64, u64, vp],
            "nsx_ipv4_hdr_csum_dev": [vp, u64, u32, u64, i32, vp, vp],
            "nsx_ipv4_hdr_verify_mask_dev": [vp, u64, u32, u64, vp, vp],
            "nsx_rx_ipv4_tcp_verify_dev": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_rx_ipv4_tcp_verify_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_rx_ipv4_tcp_verify_host": [vp, vp, u64, vp, i32],
            "nsx_rx_ipv4_tcp_verify_host_tuned": [vp, vp, u64, vp, i32, vp],
            "nsx_tcp_parse_dev": [vp, vp, u64, vp, vp],
            "nsx_rx_ipv6_tcp_verify_dev": [vp, vp, u64, vp, vp, vp],
            "nsx_rx_ipv6_tcp_verify_dev_tuned": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_rx_ipv6_tcp_verify_host": [vp, vp, u64, vp, i32],
            "nsx_rx_ipv6_tcp_verify_host_tuned": [vp, vp, u64, vp, i32, vp],
            "nsx_tcp_build_dev": [vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp],
            "nsx_tcp_layout_host": [vp, vp, u64, vp],
            "nsx_abi_version": [],
            "nsx_device_count": [ctypes.POINTER(i32)],
            # include/nsx_tune.h (per-call overrides)
            "nsx_csum_fixed_dev_tuned": [vp, u64, u32, u64, vp, vp, vp, vp],
            "nsx_csum_ragged_dev_tuned": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_verify_ragged_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_tcp_build_dev_tuned": [vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp],
            "nsx_ipv4_hdr_csum_dev_tuned": [vp, u64, u32, u64, i32, vp, vp, vp],
            "nsx_ipv4_hdr_verify_mask_dev_tuned": [vp, u64, u32, u64, vp, vp, vp],
            "nsx_csum_fixed_host_tuned": [vp, u64, u32, u64, vp, vp, i32, vp],
            "nsx_csum_ragged_host_tuned": [vp, vp, u64, vp, vp, i32, vp],
            "nsx_tcp_build_host": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, i32],
            "nsx_tcp_build_host_tuned": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, i32, vp],
            "nsx_tx_layout_host": [vp, vp, u64, u32, vp],
            "nsx_tx_ipv4_tcp_build_dev": [vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp],
            "nsx_tx_ipv6_tcp_build_dev": [vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp],
            "nsx_tx_ipv4_tcp_build_dev_tuned": [vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, vp],
            "nsx_tx_ipv6_tcp_build_dev_tuned": [vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, vp],
            "nsx_tx_ipv4_tcp_build_host": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, i32],
            "nsx_tx_ipv6_tcp_build_host": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, i32],
            "nsx_tx_ipv4_tcp_build_host_tuned": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, i32, vp],
            "nsx_tx_ipv6_tcp_build_host_tuned": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, i32, vp],
            "nsx_tso_count_host": [vp, vp, u64, vp],
            "nsx_tso_layout_host": [vp, vp, vp, vp, u64, u32, vp, vp],
            "nsx_tso_ipv4_tcp_build_dev": [vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp],
            "nsx_tso_ipv6_tcp_build_dev": [vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp],
            "nsx_tso_ipv4_tcp_build_dev_tuned": [vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_tso_ipv6_tcp_build_dev_tuned": [vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_tso_ipv4_tcp_build_host": [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, i32],
            "nsx_tso_ipv6_tcp_build_host": [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, i32],
            "nsx_tso_ipv4_tcp_build_host_tuned": [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, i32, vp],
            "nsx_tso_ipv6_tcp_build_host_tuned": [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, i32, vp],
            "nsx_gro_work_bytes": [u64, ctypes.POINTER(u64)],
            "nsx_gro_ipv4_tcp_dev": [vp, vp, u64, vp, vp, vp, u64, vp],
            "nsx_gro_ipv6_tcp_dev": [vp, vp, u64, vp, vp, vp, u64, vp],
            "nsx_gro_ipv4_tcp_dev_tuned": [vp, vp, u64, vp, vp, vp, u64, vp, vp],
            "nsx_gro_ipv6_tcp_dev_tuned": [vp, vp, u64, vp, vp, vp, u64, vp, vp],
            "nsx_gro_flow_work_bytes": [u64, ctypes.POINTER(u64)],
            "nsx_gro_flow_ipv4_tcp_dev": [vp, vp, u64, vp, vp, vp, vp, u64, vp],
            "nsx_gro_flow_ipv6_tcp_dev": [vp, vp, u64, vp, vp, vp, vp, u64, vp],
            "nsx_gro_flow_ipv4_tcp_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, u64, vp, vp],
            "nsx_gro_flow_ipv6_tcp_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, u64, vp, vp],
            "nsx_nat_table_slots": [u64, ctypes.POINTER(u64)],
            "nsx_nat_table_build_host": [u32, vp, vp, u64, vp, u64],
            "nsx_nat_ipv4_tcp_rewrite_dev": [vp, vp, u64, vp, vp, u64, u32, vp, vp],
            "nsx_nat_ipv6_tcp_rewrite_dev": [vp, vp, u64, vp, vp, u64, u32, vp, vp],
            "nsx_udp_layout_host": [vp, u64, u32, vp],
            "nsx_udp_uso_layout_host": [vp, vp, vp, u64, u32, vp, vp],
            "nsx_udp_tx_ipv4_build_dev": [vp, vp, vp, vp, u64, u64, u32, vp, vp, vp, vp],
            "nsx_udp_tx_ipv6_build_dev": [vp, vp, vp, vp, u64, u64, u32, vp, vp, vp, vp],
            "nsx_udp_tx_ipv4_build_dev_tuned": [vp, vp, vp, vp, u64, u64, u32, vp, vp, vp, vp, vp],
            "nsx_udp_tx_ipv6_build_dev_tuned": [vp, vp, vp, vp, u64, u64, u32, vp, vp, vp, vp, vp],
            "nsx_udp_uso_ipv4_build_dev": [vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, vp],
            "nsx_udp_uso_ipv6_build_dev": [vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, vp],
            "nsx_udp_uso_ipv4_build_dev_tuned": [vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, vp, vp],
            "nsx_udp_uso_ipv6_build_dev_tuned": [vp, vp, vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, vp, vp],
            "nsx_udp_rx_ipv4_verify_dev": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_udp_rx_ipv4_verify_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_udp_rx_ipv6_verify_dev": [vp, vp, u64, vp, vp, vp],
            "nsx_udp_rx_ipv6_verify_dev_tuned": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_ugro_work_bytes": [u64, ctypes.POINTER(u64)],
            "nsx_ugro_flow_work_bytes": [u64, ctypes.POINTER(u64)],
            "nsx_ugro_ipv4_dev": [vp, vp, u64, vp, vp, vp, u64, vp],
            "nsx_ugro_ipv6_dev": [vp, vp, u64, vp, vp, vp, u64, vp],
            "nsx_ugro_ipv4_dev_tuned": [vp, vp, u64, vp, vp, vp, u64, vp, vp],
            "nsx_ugro_ipv6_dev_tuned": [vp, vp, u64, vp, vp, vp, u64, vp, vp],
            "nsx_ugro_flow_ipv4_dev": [vp, vp, u64, vp, vp, vp, vp, u64, vp],
            "nsx_ugro_flow_ipv6_dev": [vp, vp, u64, vp, vp, vp, vp, u64, vp],
            "nsx_ugro_flow_ipv4_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, u64, vp, vp],
            "nsx_ugro_flow_ipv6_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, u64, vp, vp],
            "nsx_frag_count_host": [vp, vp, u64, vp],
            "nsx_frag_layout_host": [vp, vp, vp, u64, vp, vp],
            "nsx_frag_ipv4_dev": [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp],
            "nsx_frag_ipv4_dev_tuned": [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_reasm_work_bytes": [u64, ctypes.POINTER(u64)],
            "nsx_reasm_ipv4_dev": [vp, vp, u64, vp, vp, vp, u64, vp],
            "nsx_reasm_ipv4_dev_tuned": [vp, vp, u64, vp, vp, vp, u64, vp, vp],
            "nsx_icmp_err_work_bytes": [u64, ctypes.POINTER(u64)],
            "nsx_icmp_err_ipv4_dev": [vp, vp, u64, vp, vp, vp, vp, vp, u64, vp],
            "nsx_icmp_err_ipv6_dev": [vp, vp, u64, vp, vp, vp, vp, vp, u64, vp],
            "nsx_icmp_err_ipv4_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp],
            "nsx_icmp_err_ipv6_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp],
            "nsx_icmp_req_frag_dev": [vp, vp, u64, vp, vp, vp],
            "nsx_icmp_req_ttl_ipv4_dev": [vp, vp, u64, vp, u32, vp, vp, vp],
            "nsx_icmp_req_ttl_ipv6_dev": [vp, vp, u64, vp, u32, vp, vp, vp],
            "nsx_icmp_rx_ipv4_verify_dev": [vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_icmp_rx_ipv4_verify_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp, vp],
            "nsx_icmp_rx_ipv6_verify_dev": [vp, vp, u64, vp, vp, vp, vp],
            "nsx_icmp_rx_ipv6_verify_dev_tuned": [vp, vp, u64, vp, vp, vp, vp, vp],
            "nsx_icmp_echo_reply_ipv4_dev": [vp, vp, u64, vp, u32, vp, vp],
            "nsx_icmp_echo_reply_ipv6_dev": [vp, vp, u64, vp, u32, vp, vp],
            "nsx_fixed_launch_count": [u64, u32, u64, vp, ctypes.POINTER(u64)],
            "nsx_ipv4_hdr_launch_count": [vp, u64, u32, u64, vp, ctypes.POINTER(u64)],
        }
        # present since ABI round 6, and the transmit pass since its own change; an older library (same-box A/B against a
        # previous build) lacks them
        optional = {"nsx_stream_release", "nsx_deal_sets_in_use"} | \
            {k for k in sig if k.startswith(("nsx_tx_", "nsx_tso_", "nsx_gro_", "nsx_nat_", "nsx_udp_", "nsx_ugro_", "nsx_frag_",
                                           "nsx_reasm_", "nsx_icmp_"))}
        for name, args in sig.items():
            if name in optional and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.argtypes = args
            f.restype = ctypes.c_int
        L.nsx_tcp_wire_len.argtypes = [u64, u64]
        L.nsx_tcp_wire_len.restype = ctypes.c_uint64
        L.nsx_strerror.argtypes = [i32]
        L.nsx_strerror.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != NSX_OK:
        raise NsxError(rc, what)


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dev_ptr(t):
    """A device tensor's address for the C call (a host tensor is refused: the device entry points take HBM
    pointers). Called after every _span check of the wrapper, so extent errors are reported first."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f"must be a device (HIP) tensor, got one on {t.device}")
    return ctypes.c_void_p(t.data_ptr())


def _span(t, nbytes: int, what: str, elem: int | None = None):
    """The C ABI takes bare device pointers and cannot see extents, so every device wrapper checks its tensors
    here, before the C call: contiguous, `elem`-byte elements (when given), at least `nbytes` bytes (_dev_ptr then
    refuses host tensors). An undersized tensor would otherwise be an out-of-bounds device access. (Data-dependent extents — a ragged
    batch's last offset — live in device memory and are not read here: that would synchronise the stream.)"""
    if t is None:
        return
    if not t.is_contiguous():
        raise ValueError(f"{what}: tensor must be contiguous")
    if elem is not None and t.element_size() != elem:
        raise ValueError(f"{what}: needs {elem}-byte elements, got {t.dtype}")
    have = t.numel() * t.element_size()
    if have < nbytes:
        raise ValueError(f"{what}: {have} B given, {nbytes} B needed")


def _count(offsets, what: str) -> int:
    """n from an (n+1)-entry offsets tensor of 8-byte elements."""
    _span(offsets, 8, what, elem=8)
    return offsets.numel() - 1


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


# ---------------------------------------------------------------------------
# host-side API
# ---------------------------------------------------------------------------
def abi_version() -> int:
    return lib().nsx_abi_version()


def device_count() -> int:
    c = ctypes.c_int(0)
    _check(lib().nsx_device_count(ctypes.byref(c)), "nsx_device_count")
    return c.value


def csum16(prefix: bytes, seg: bytes) -> int:
    """computeChecksum (tcp.go:72-95): raw one's-complement sum over prefix ‖ seg."""
    p = np.frombuffer(bytes(prefix), np.uint8) if prefix else None
    s = np.frombuffer(bytes(seg), np.uint8) if seg else None
    out = ctypes.c_uint16(0)
    _check(lib().nsx_csum16(_np_ptr(p), len(prefix), _np_ptr(s), len(seg), ctypes.byref(out)), "nsx_csum16")
    return out.value


def field(raw: int) -> int:
    return (~raw) & 0xFFFF


def verify(raw: int) -> bool:
    return raw == 0xFFFF


def shard_plan(n: int, parts: int, offsets: np.ndarray | None = None) -> np.ndarray:
    b = np.zeros(parts + 1, np.uint64)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    _check(lib().nsx_shard_plan(_np_ptr(off), n, parts, _np_ptr(b)), "nsx_shard_plan")
    return b


def stream_release(stream) -> None:
    """nsx_stream_release: return a stream's deal counters (call after it has drained, before destroying it).
    `stream`: a torch stream, or a raw handle value (int)."""
    h = stream if isinstance(stream, int) else stream.cuda_stream
    _check(lib().nsx_stream_release(ctypes.c_void_p(h)), "nsx_stream_release")


def deal_sets_in_use() -> int:
    """Per-stream deal counter sets given out on the current device (nsx_deal_sets_in_use)."""
    c = ctypes.c_uint32(0)
    _check(lib().nsx_deal_sets_in_use(ctypes.byref(c)), "nsx_deal_sets_in_use")
    return c.value


def ipv4_hdr_launch_count(buf, stride: int, n: int, hdr_off: int = 0, tune=None) -> int:
    """Kernel launches one IPv4 header call makes for this batch on the current device."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_ipv4_hdr_launch_count(ctypes.c_void_p(buf.data_ptr()), stride, hdr_off, n, _tune(tune),
                                           ctypes.byref(c)), "nsx_ipv4_hdr_launch_count")
    return c.value


def fixed_launch_count(stride: int, seg_len: int, n: int, tune=None) -> int:
    """Kernel launches one fixed_dev call makes for this batch on the current device."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_fixed_launch_count(stride, seg_len, n, _tune(tune), ctypes.byref(c)), "nsx_fixed_launch_count")
    return c.value


def fixed_host(buf: np.ndarray, stride: int, seg_len: int, n: int, partial: np.ndarray | None = None,
               num_gpus: int = 0, tune=None) -> np.ndarray:
    buf = np.ascontiguousarray(buf, np.uint8)
    out = np.empty(n, np.uint16)
    part = None if partial is None else np.ascontiguousarray(partial, np.uint32)
    if n > 0 and buf.size < (n - 1) * stride + seg_len:
        raise ValueError(f"fixed_host buf: {buf.size} B given, {(n - 1) * stride + seg_len} B needed")
    if part is not None and part.size < n:
        raise ValueError(f"fixed_host partial: {part.size} entries for {n} segments")
    _check(lib().nsx_csum_fixed_host_tuned(_np_ptr(buf), stride, seg_len, n, _np_ptr(part), _np_ptr(out), num_gpus,
                                           _tune(tune)), "nsx_csum_fixed_host")
    return out


def ragged_host(buf: np.ndarray, offsets: np.ndarray, partial: np.ndarray | None = None,
                num_gpus: int = 0, tune=None) -> np.ndarray:
    buf = np.ascontiguousarray(buf, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = offsets.size - 1
    out = np.empty(max(n, 0), np.uint16)
    part = None if partial is None else np.ascontiguousarray(partial, np.uint32)
    if n > 0 and buf.size < int(offsets[-1]):
        raise ValueError(f"ragged_host buf: {buf.size} B given, offsets end at {int(offsets[-1])}")
    if part is not None and part.size < n:
        raise ValueError(f"ragged_host partial: {part.size} entries for {n} segments")
    _check(lib().nsx_csum_ragged_host_tuned(_np_ptr(buf), _np_ptr(offsets), n, _np_ptr(part), _np_ptr(out), num_gpus,
                                            _tune(tune)), "nsx_csum_ragged_host")
    return out


def rx_ipv4_tcp_verify_host(buf: np.ndarray, offsets: np.ndarray, num_gpus: int = 0, tune=None,
                            ipver: int = 4) -> np.ndarray:
    """Fused receive pass over host-resident datagrams (IPv4, or IPv6 with ipver=6): the validity bitmask
    (uint64[ceil(n/64)])."""
    buf = np.ascontiguousarray(buf, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = offsets.size - 1
    mask = np.zeros((max(n, 0) + 63) // 64, np.uint64)
    if n > 0 and buf.size < int(offsets[-1]):
        raise ValueError(f"rx host buf: {buf.size} B given, offsets end at {int(offsets[-1])}")
    name = "nsx_rx_ipv6_tcp_verify_host" if ipver == 6 else "nsx_rx_ipv4_tcp_verify_host"
    _check(getattr(lib(), name + "_tuned")(_np_ptr(buf), _np_ptr(offsets), n, _np_ptr(mask), num_gpus, _tune(tune)),
           name)
    return mask


def rx_ipv6_tcp_verify_host(buf: np.ndarray, offsets: np.ndarray, num_gpus: int = 0, tune=None) -> np.ndarray:
    return rx_ipv4_tcp_verify_host(buf, offsets, num_gpus, tune, ipver=6)


class PinnedBuffer:
    """nsx_alloc_pinned-backed numpy view (DMA-registered host memory)."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        _check(lib().nsx_alloc_pinned(nbytes, ctypes.byref(p)), "nsx_alloc_pinned")
        self._p = p
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p.value)) if nbytes else \
            np.zeros(0, np.uint8)

    def free(self):
        if self._p:
            _check(lib().nsx_free_pinned(self._p), "nsx_free_pinned")
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# device-side API (torch tensors as HBM buffers)
# ---------------------------------------------------------------------------
def fixed_dev(buf, stride: int, seg_len: int, n: int, partial=None, out=None, stream=None, tune=None):
    import torch
    if out is None:
        out = torch.empty(n, dtype=torch.int16, device=buf.device)  # u16 bits
    _span(buf, (n - 1) * stride + seg_len if n > 0 else 0, "fixed_dev buf")
    _span(partial, 4 * n, "fixed_dev partial", elem=4)
    _span(out, 2 * n, "fixed_dev out", elem=2)
    _check(lib().nsx_csum_fixed_dev_tuned(_dev_ptr(buf), stride, seg_len, n, _dev_ptr(partial), _dev_ptr(out),
                                          _stream(stream), _tune(tune)), "nsx_csum_fixed_dev")
    return out


def ragged_dev(buf, offsets, partial=None, out=None, stream=None, tune=None):
    import torch
    n = _count(offsets, "ragged_dev offsets")
    if out is None:
        out = torch.empty(max(n, 0), dtype=torch.int16, device=offsets.device)  # u16 bits
    _span(buf, 0, "ragged_dev buf")
    _span(partial, 4 * n, "ragged_dev partial", elem=4)
    _span(out, 2 * n, "ragged_dev out", elem=2)
    _check(lib().nsx_csum_ragged_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(partial), _dev_ptr(out),
                                           _stream(stream), _tune(tune)), "nsx_csum_ragged_dev")
    return out


def verify_ragged_dev(buf, offsets, partial=None, raw=None, stream=None, tune=None, ok=None):
    import torch
    n = _count(offsets, "verify_ragged_dev offsets")
    if ok is None:
        ok = torch.empty(max(n, 0), dtype=torch.uint8, device=offsets.device)
    _span(ok, n, "verify_ragged_dev ok")
    _span(buf, 0, "verify_ragged_dev buf")
    _span(partial, 4 * n, "verify_ragged_dev partial", elem=4)
    _span(raw, 2 * n, "verify_ragged_dev raw", elem=2)
    _check(lib().nsx_verify_ragged_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(partial), _dev_ptr(ok),
                                             _dev_ptr(raw), _stream(stream), _tune(tune)), "nsx_verify_ragged_dev")
    return ok


def pseudo_ipv4_partial_dev(src, dst, length, proto: int = 6, out=None, stream=None):
    import torch
    n = length.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=length.device)  # u32 bits
    _span(length, 4 * n, "pseudo_ipv4_partial_dev length", elem=4)
    _span(src, 4 * n, "pseudo_ipv4_partial_dev src")
    _span(dst, 4 * n, "pseudo_ipv4_partial_dev dst")
    _span(out, 4 * n, "pseudo_ipv4_partial_dev out", elem=4)
    _check(lib().nsx_pseudo_ipv4_partial_dev(_dev_ptr(src), _dev_ptr(dst), _dev_ptr(length), proto, n,
                                             _dev_ptr(out), _stream(stream)), "nsx_pseudo_ipv4_partial_dev")
    return out


def pseudo_ipv6_partial_dev(src, dst, length, next_header: int = 6, out=None, stream=None):
    import torch
    n = length.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=length.device)  # u32 bits
    _span(length, 4 * n, "pseudo_ipv6_partial_dev length", elem=4)
    _span(src, 16 * n, "pseudo_ipv6_partial_dev src")
    _span(dst, 16 * n, "pseudo_ipv6_partial_dev dst")
    _span(out, 4 * n, "pseudo_ipv6_partial_dev out", elem=4)
    _check(lib().nsx_pseudo_ipv6_partial_dev(_dev_ptr(src), _dev_ptr(dst), _dev_ptr(length), next_header, n,
                                             _dev_ptr(out), _stream(stream)), "nsx_pseudo_ipv6_partial_dev")
    return out


def verify_mask_dev(raw, out=None, stream=None):
    """Bitmask of raw == 0xFFFF (tcp.go:70): int64 tensor of ceil(n/64) words."""
    import torch
    n = raw.numel()
    if out is None:
        out = torch.empty((n + 63) // 64, dtype=torch.int64, device=raw.device)  # u64 bits
    _span(raw, 2 * n, "verify_mask_dev raw", elem=2)
    _span(out, 8 * ((n + 63) // 64), "verify_mask_dev out", elem=8)
    _check(lib().nsx_verify_mask_dev(_dev_ptr(raw), n, _dev_ptr(out), _stream(stream)), "nsx_verify_mask_dev")
    return out


def ipv4_hdr_csum_dev(buf, stride: int, n: int, hdr_off: int = 0, mode: int = 0, out=None, stream=None, tune=None):
    """RFC 791 header checksums of n packets at a fixed stride (mode 0 verify, 1 fill in place)."""
    import torch
    if out is None and mode == 0:
        out = torch.empty(n, dtype=torch.int16, device=buf.device)  # u16 bits
    _span(buf, (n - 1) * stride + hdr_off + 20 if n > 0 else 0, "ipv4_hdr_csum_dev buf")
    _span(out, 2 * n, "ipv4_hdr_csum_dev out", elem=2)
    _check(lib().nsx_ipv4_hdr_csum_dev_tuned(_dev_ptr(buf), stride, hdr_off, n, mode, _dev_ptr(out), _stream(stream),
                                             _tune(tune)), "nsx_ipv4_hdr_csum_dev")
    return out


def ipv4_hdr_verify_mask_dev(buf, stride: int, n: int, hdr_off: int = 0, mask=None, stream=None, tune=None):
    """Fused IPv4 header verify into a bitmask: bit i%64 of mask[i//64] iff header i is valid."""
    import torch
    if mask is None:
        mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=buf.device)  # u64 bits
    _span(buf, (n - 1) * stride + hdr_off + 20 if n > 0 else 0, "ipv4_hdr_verify_mask_dev buf")
    _span(mask, 8 * ((n + 63) // 64), "ipv4_hdr_verify_mask_dev mask", elem=8)
    _check(lib().nsx_ipv4_hdr_verify_mask_dev_tuned(_dev_ptr(buf), stride, hdr_off, n, _dev_ptr(mask),
                                                    _stream(stream), _tune(tune)), "nsx_ipv4_hdr_verify_mask_dev")
    return mask


def rx_ipv4_tcp_verify_dev(buf, offsets, mask=None, ip_raw=None, tcp_raw=None, stream=None, tune=None):
    """Fused receive pass over packed IPv4/TCP frames: validity bitmask (+ optional raw sums)."""
    import torch
    n = _count(offsets, "rx_ipv4_tcp_verify_dev offsets")
    if mask is None:
        mask = torch.empty((max(n, 0) + 63) // 64, dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(buf, 0, "rx_ipv4_tcp_verify_dev buf")
    _span(mask, 8 * ((n + 63) // 64), "rx_ipv4_tcp_verify_dev mask", elem=8)
    _span(ip_raw, 2 * n, "rx_ipv4_tcp_verify_dev ip_raw", elem=2)
    _span(tcp_raw, 2 * n, "rx_ipv4_tcp_verify_dev tcp_raw", elem=2)
    _check(lib().nsx_rx_ipv4_tcp_verify_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(mask),
                                                  _dev_ptr(ip_raw), _dev_ptr(tcp_raw), _stream(stream), _tune(tune)),
           "nsx_rx_ipv4_tcp_verify_dev")
    return mask


def rx_ipv6_tcp_verify_dev(buf, offsets, mask=None, tcp_raw=None, stream=None, tune=None):
    """Fused receive pass over packed IPv6/TCP packets: validity bitmask (+ optional raw TCP sums)."""
    import torch
    n = _count(offsets, "rx_ipv6_tcp_verify_dev offsets")
    if mask is None:
        mask = torch.empty((max(n, 0) + 63) // 64, dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(buf, 0, "rx_ipv6_tcp_verify_dev buf")
    _span(mask, 8 * ((n + 63) // 64), "rx_ipv6_tcp_verify_dev mask", elem=8)
    _span(tcp_raw, 2 * n, "rx_ipv6_tcp_verify_dev tcp_raw", elem=2)
    _check(lib().nsx_rx_ipv6_tcp_verify_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(mask),
                                                  _dev_ptr(tcp_raw), _stream(stream), _tune(tune)),
           "nsx_rx_ipv6_tcp_verify_dev")
    return mask


BUILD_FIELDS = (("src_port", 2), ("dst_port", 2), ("seq_num", 4), ("ack_num", 4), ("offset", 1), ("control", 1),
                ("window", 2), ("urgent_ptr", 2))  # nsx_tcp_hdr_soa members and their element sizes


class TcpHdrSoA(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in BUILD_FIELDS]


PARSE_FIELDS = (("src_port", "int16"), ("dst_port", "int16"), ("seq_num", "int32"), ("ack_num", "int32"),
                ("offset", "uint8"), ("control", "uint8"), ("window", "int16"), ("checksum", "int16"),
                ("urgent_ptr", "int16"), ("data_off", "int64"), ("n_options", "uint8"), ("status", "uint8"))
PARSE_OK, PARSE_SHORT, PARSE_OFFSET, PARSE_OPTION_RANGE, PARSE_OPTION_KIND = 0, 1, 2, 3, 4


class TcpParsedSoA(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in PARSE_FIELDS]


def tcp_parse_dev(buf, offsets, fields=None, want=None, stream=None) -> dict:
    """parseSegment (tcp.go:130-185) over the segments buf[offsets[i], offsets[i+1]) into device tensors (dict
    by field; `want` = the field names to produce, default all; `fields` = caller tensors to fill)."""
    import torch
    n = _count(offsets, "tcp_parse_dev offsets")
    names = [k for k, _ in PARSE_FIELDS] if want is None else list(want)
    out = dict(fields or {})
    for k, dt in PARSE_FIELDS:
        if k in names and k not in out:
            out[k] = torch.empty(max(n, 0), dtype=getattr(torch, dt), device=offsets.device)
    _span(buf, 0, "tcp_parse_dev buf")
    for k, dt in PARSE_FIELDS:
        size = np.dtype(dt).itemsize
        _span(out.get(k), size * n, f"tcp_parse_dev {k}", elem=size)
    soa =TcpParsedSoA(*[_dev_ptr(out.get(k)) for k, _ in PARSE_FIELDS])
    _check(lib().nsx_tcp_parse_dev(_dev_ptr(buf), _dev_ptr(offsets), n, ctypes.byref(soa), _stream(stream)),
           "nsx_tcp_parse_dev")
    return out


def tcp_wire_len(opt_len: int, data_len: int) -> int:
    return lib().nsx_tcp_wire_len(opt_len, data_len)


def tcp_layout_host(data_off: np.ndarray, opt_off: np.ndarray | None = None) -> np.ndarray:
    data_off = np.ascontiguousarray(data_off, np.uint64)
    n = data_off.size - 1
    out = np.zeros(n + 1, np.uint64)
    oo = None if opt_off is None else np.ascontiguousarray(opt_off, np.uint64)
    _check(lib().nsx_tcp_layout_host(_np_ptr(oo), _np_ptr(data_off), n, _np_ptr(out)), "nsx_tcp_layout_host")
    return out


def tcp_build_dev(fields: dict, data, data_off, out, out_off, opts=None, opt_off=None, partial=None, raw=None,
                  stream=None, tune=None):
    """Fused segment.bytes() + checksum + field write (fields: dict of device tensors; a missing or None
    "offset" computes byte 12 on the device as computeOffset() does, tcp.go:59-66)."""
    n = _count(data_off, "tcp_build_dev data_off")
    for k, size in BUILD_FIELDS:
        if fields.get(k) is None and k != "offset":  # only byte 12 may be computed on the device
            raise ValueError(f"tcp_build_dev: header field {k!r} missing")
        _span(fields.get(k), size * n, f"tcp_build_dev {k}", elem=size)
    _span(data, 0, "tcp_build_dev data")
    _span(out_off, 8 * (n + 1), "tcp_build_dev out_off", elem=8)
    _span(out, 0, "tcp_build_dev out")
    _span(opt_off, 8 * (n + 1), "tcp_build_dev opt_off", elem=8)
    if opt_off is not None and opts is None:
        raise ValueError("tcp_build_dev: opt_off given without opts")
    _span(opts, 0, "tcp_build_dev opts")
    _span(partial, 4 * n, "tcp_build_dev partial", elem=4)
    _span(raw, 2 * n, "tcp_build_dev raw", elem=2)
    soa = TcpHdrSoA(*[_dev_ptr(fields.get(k)) for k, _ in BUILD_FIELDS])
    _check(lib().nsx_tcp_build_dev_tuned(ctypes.byref(soa), _dev_ptr(opts), _dev_ptr(opt_off), _dev_ptr(data),
                                         _dev_ptr(data_off), data.numel(), _dev_ptr(partial), n, _dev_ptr(out),
                                         _dev_ptr(out_off), _dev_ptr(raw), _stream(stream), _tune(tune)),
           "nsx_tcp_build_dev")
    return out


_BUILD_NP = {"src_port": np.uint16, "dst_port": np.uint16, "seq_num": np.uint32, "ack_num": np.uint32,
             "offset": np.uint8, "control": np.uint8, "window": np.uint16, "urgent_ptr": np.uint16}


def tcp_build_host(fields: dict, data: np.ndarray, data_off: np.ndarray, out_off: np.ndarray | None = None,
                   opts: np.ndarray | None = None, opt_off: np.ndarray | None = None,
                   partial: np.ndarray | None = None, out: np.ndarray | None = None, want_raw: bool = True,
                   num_gpus: int = 0, tune=None):
    """The fused sender pass over host-resident segments (nsx_tcp_build_host): fields = dict of host arrays (a
    missing or None "offset" is computed on the device, tcp.go:59-66); out_off defaults to nsx_tcp_layout_host;
    out (host uint8, e.g. a PinnedBuffer's array) is allocated when not given. Returns (out, raw or None)."""
    data = np.ascontiguousarray(data, np.uint8)
    data_off = np.ascontiguousarray(data_off, np.uint64)
    n = data_off.size - 1
    cols = {}
    for k, _ in BUILD_FIELDS:
        v = fields.get(k)
        if v is None:
            if k != "offset":
                raise ValueError(f"tcp_build_host: header field {k!r} missing")
            continue
        v = np.ascontiguousarray(v).view(_BUILD_NP[k]) if np.asarray(v).dtype.itemsize == np.dtype(_BUILD_NP[k]).itemsize \
            else np.ascontiguousarray(v, _BUILD_NP[k])
        if v.size < n:
            raise ValueError(f"tcp_build_host {k}: {v.size} entries for {n} segments")
        cols[k] = v
    oo = None if opt_off is None else np.ascontiguousarray(opt_off, np.uint64)
    if oo is not None and opts is None:
        raise ValueError("tcp_build_host: opt_off given without opts")
    ob = None if opts is None else (np.ascontiguousarray(opts, np.uint8) if len(opts) else np.zeros(1, np.uint8))
    if out_off is None:
        out_off = tcp_layout_host(data_off, oo)
    out_off = np.ascontiguousarray(out_off, np.uint64)
    if n > 0 and data.size < int(data_off[-1]):
        raise ValueError(f"tcp_build_host data: {data.size} B given, data_off ends at {int(data_off[-1])}")
    if oo is not None and n > 0 and ob.size < int(oo[-1]):
        raise ValueError(f"tcp_build_host opts: {ob.size} B given, opt_off ends at {int(oo[-1])}")
    if out is None:
        out = np.zeros(int(out_off[-1]) if n > 0 else 0, np.uint8)
    # the C call writes the images contiguously from out's first byte: a strided view, or a view of wider elements,
    # would be written past
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous:
        raise ValueError("tcp_build_host out: needs a C-contiguous uint8 array")
    if n > 0 and out.size < int(out_off[-1]):
        raise ValueError(f"tcp_build_host out: {out.size} B given, out_off ends at {int(out_off[-1])}")
    part = None if partial is None else np.ascontiguousarray(partial, np.uint32)
    if part is not None and part.size < n:
        raise ValueError(f"tcp_build_host partial: {part.size} entries for {n} segments")
    raw = np.empty(max(n, 0), np.uint16) if want_raw else None
    soa = TcpHdrSoA(*[_np_ptr(cols.get(k)) for k, _ in BUILD_FIELDS])
    _check(lib().nsx_tcp_build_host_tuned(ctypes.byref(soa), _np_ptr(ob), _np_ptr(oo), _np_ptr(data),
                                          _np_ptr(data_off), _np_ptr(part), n, _np_ptr(out), _np_ptr(out_off),
                                          _np_ptr(raw), num_gpus, _tune(tune)), "nsx_tcp_build_host")
    return out, raw


# ---------------------------------------------------------------------------
# fused transmit pass: whole IPv4 / IPv6 datagrams (nsx_tx_*)
# ---------------------------------------------------------------------------
IP_FIELDS = ("src", "dst", "ident", "ttl", "tclass", "flow")  # nsx_ip_hdr_soa members


class IpHdrSoA(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in IP_FIELDS]


def _ip_sizes(ipver: int) -> dict:
    """Bytes per frame of each nsx_ip_hdr_soa array."""
    if ipver not in (4, 6):
        raise ValueError(f"ipver must be 4 or 6, got {ipver}")
    alen = 4 if ipver == 4 else 16
    return {"src": alen, "dst": alen, "ident": 2, "ttl": 1, "tclass": 1, "flow": 4}


def tx_layout_host(data_off: np.ndarray, opt_off: np.ndarray | None = None, ip_hdr_len: int = 20) -> np.ndarray:
    """nsx_tx_layout_host: packed 4-aligned frame offsets, out_off[i] = Σ_{j<i} round_up4(ip_hdr_len + wire_j)
    (ip_hdr_len 20 for IPv4, 40 for IPv6)."""
    data_off = np.ascontiguousarray(data_off, np.uint64)
    n = data_off.size - 1
    out = np.zeros(n + 1, np.uint64)
    oo = None if opt_off is None else np.ascontiguousarray(opt_off, np.uint64)
    if oo is not None and oo.size < n + 1:
        raise ValueError(f"tx_layout_host opt_off: {oo.size} entries for {n} frames")
    _check(lib().nsx_tx_layout_host(_np_ptr(oo), _np_ptr(data_off), n, ip_hdr_len, _np_ptr(out)), "nsx_tx_layout_host")
    return out


def _tx_build_dev(ipver: int, ip: dict, fields: dict, data, data_off, out, out_off, opts, opt_off, raw, stream, tune):
    what = f"tx_ipv{ipver}_tcp_build_dev"
    n = _count(data_off, f"{what} data_off")
    sizes = _ip_sizes(ipver)
    for k in ("src", "dst"):
        if ip.get(k) is None:
            raise ValueError(f"{what}: address array {k!r} missing")
    for k in IP_FIELDS:
        _span(ip.get(k), sizes[k] * n, f"{what} {k}", elem=None if k in ("src", "dst") else sizes[k])
    for k, size in BUILD_FIELDS:
        if fields.get(k) is None and k != "offset":  # only byte 12 may be computed on the device
            raise ValueError(f"{what}: header field {k!r} missing")
        _span(fields.get(k), size * n, f"{what} {k}", elem=size)
    _span(data, 0, f"{what} data")
    _span(out_off, 8 * (n + 1), f"{what} out_off", elem=8)
    # the frame lengths are in device memory; the least n frames can take is an IP and a TCP header each
    _span(out, max(n, 0) * (40 if ipver == 4 else 60), f"{what} out", elem=1)
    _span(opt_off, 8 * (n + 1), f"{what} opt_off", elem=8)
    if opt_off is not None and opts is None:
        raise ValueError(f"{what}: opt_off given without opts")
    _span(opts, 0, f"{what} opts")
    _span(raw, 2 * n, f"{what} raw", elem=2)
    ipsoa = IpHdrSoA(*[_dev_ptr(ip.get(k)) for k in IP_FIELDS])
    soa = TcpHdrSoA(*[_dev_ptr(fields.get(k)) for k, _ in BUILD_FIELDS])
    fn = getattr(lib(), f"nsx_tx_ipv{ipver}_tcp_build_dev_tuned")
    _check(fn(ctypes.byref(ipsoa), ctypes.byref(soa), _dev_ptr(opts), _dev_ptr(opt_off), _dev_ptr(data),
              _dev_ptr(data_off), data.numel(), n, _dev_ptr(out), _dev_ptr(out_off), _dev_ptr(raw), _stream(stream),
              _tune(tune)), f"nsx_{what}")
    return out


def tx_ipv4_tcp_build_dev(ip: dict, fields: dict, data, data_off, out, out_off, opts=None, opt_off=None, raw=None,
                          stream=None, tune=None):
    """Fused transmit pass: whole IPv4 datagrams (header checksum and TCP checksum in place) at out + out_off[i].
    ip: dict of device tensors src, dst (uint8, 4 B per frame) and optionally ident (2 B), ttl (1 B); fields,
    opts and the layout rule as tcp_build_dev; raw (optional) receives the TCP raw sums."""
    return _tx_build_dev(4, ip, fields, data, data_off, out, out_off, opts, opt_off, raw, stream, tune)


def tx_ipv6_tcp_build_dev(ip: dict, fields: dict, data, data_off, out, out_off, opts=None, opt_off=None, raw=None,
                          stream=None, tune=None):
    """The same for IPv6: src, dst 16 B per frame; optionally ttl (hop limit), tclass (1 B), flow (4 B)."""
    return _tx_build_dev(6, ip, fields, data, data_off, out, out_off, opts, opt_off, raw, stream, tune)


_IP_NP = {"src": np.uint8, "dst": np.uint8, "ident": np.uint16, "ttl": np.uint8, "tclass": np.uint8, "flow": np.uint32}


def _tx_build_host(ipver: int, ip: dict, fields: dict, data, data_off, out_off, opts, opt_off, out, want_raw, num_gpus,
                   tune):
    what = f"tx_ipv{ipver}_tcp_build_host"
    data = np.ascontiguousarray(data, np.uint8)
    data_off = np.ascontiguousarray(data_off, np.uint64)
    n = data_off.size - 1
    sizes = _ip_sizes(ipver)
    ipc = {}
    for k in IP_FIELDS:
        v = ip.get(k)
        if v is None:
            if k in ("src", "dst"):
                raise ValueError(f"{what}: address array {k!r} missing")
            continue
        v = np.ascontiguousarray(v, _IP_NP[k])
        if v.nbytes < sizes[k] * n:
            raise ValueError(f"{what} {k}: {v.nbytes} B given, {sizes[k] * n} B needed")
        ipc[k] = v
    cols = {}
    for k, _ in BUILD_FIELDS:
        v = fields.get(k)
        if v is None:
            if k != "offset":
                raise ValueError(f"{what}: header field {k!r} missing")
            continue
        v = np.ascontiguousarray(v, _BUILD_NP[k])
        if v.size < n:
            raise ValueError(f"{what} {k}: {v.size} entries for {n} frames")
        cols[k] = v
    oo = None if opt_off is None else np.ascontiguousarray(opt_off, np.uint64)
    if oo is not None and opts is None:
        raise ValueError(f"{what}: opt_off given without opts")
    if oo is not None and oo.size < n + 1:
        raise ValueError(f"{what} opt_off: {oo.size} entries for {n} frames")
    ob = None if opts is None else (np.ascontiguousarray(opts, np.uint8) if len(opts) else np.zeros(1, np.uint8))
    if out_off is None:
        out_off = tx_layout_host(data_off, oo, 20 if ipver == 4 else 40)
    out_off = np.ascontiguousarray(out_off, np.uint64)
    if out_off.size < n + 1:
        raise ValueError(f"{what} out_off: {out_off.size} entries for {n} frames")
    if n > 0 and data.size < int(data_off[-1]):
        raise ValueError(f"{what} data: {data.size} B given, data_off ends at {int(data_off[-1])}")
    if oo is not None and n > 0 and ob.size < int(oo[-1]):
        raise ValueError(f"{what} opts: {ob.size} B given, opt_off ends at {int(oo[-1])}")
    if out is None:
        out = np.zeros(int(out_off[-1]) if n > 0 else 0, np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous:
        raise ValueError(f"{what} out: needs a C-contiguous uint8 array")
    if n > 0 and out.size < int(out_off[n]):
        raise ValueError(f"{what} out: {out.size} B given, out_off ends at {int(out_off[n])}")
    raw = np.empty(max(n, 0), np.uint16) if want_raw else None
    ipsoa = IpHdrSoA(*[_np_ptr(ipc.get(k)) for k in IP_FIELDS])
    soa = TcpHdrSoA(*[_np_ptr(cols.get(k)) for k, _ in BUILD_FIELDS])
    fn = getattr(lib(), f"nsx_tx_ipv{ipver}_tcp_build_host_tuned")
    _check(fn(ctypes.byref(ipsoa), ctypes.byref(soa), _np_ptr(ob), _np_ptr(oo), _np_ptr(data), _np_ptr(data_off), n,
              _np_ptr(out), _np_ptr(out_off), _np_ptr(raw), num_gpus, _tune(tune)), f"nsx_{what}")
    return out, raw


def tx_ipv4_tcp_build_host(ip: dict, fields: dict, data: np.ndarray, data_off: np.ndarray,
                           out_off: np.ndarray | None = None, opts: np.ndarray | None = None,
                           opt_off: np.ndarray | None = None, out: np.ndarray | None = None, want_raw: bool = True,
                           num_gpus: int = 0, tune=None):
    """The fused transmit pass over host-resident inputs (nsx_tx_ipv4_tcp_build_host): ip and fields are dicts of
    host arrays; out_off defaults to nsx_tx_layout_host. Returns (out, raw or None)."""
    return _tx_build_host(4, ip, fields, data, data_off, out_off, opts, opt_off, out, want_raw, num_gpus, tune)


def tx_ipv6_tcp_build_host(ip: dict, fields: dict, data: np.ndarray, data_off: np.ndarray,
                           out_off: np.ndarray | None = None, opts: np.ndarray | None = None,
                           opt_off: np.ndarray | None = None, out: np.ndarray | None = None, want_raw: bool = True,
                           num_gpus: int = 0, tune=None):
    return _tx_build_host(6, ip, fields, data, data_off, out_off, opts, opt_off, out, want_raw, num_gpus, tune)


# ---------------------------------------------------------------------------
# segmentation offload on the transmit pass: super-segments in, frames out (nsx_tso_*)
# ---------------------------------------------------------------------------
def _tso_host_args(data_off, mss, what: str):
    data_off = np.ascontiguousarray(data_off, np.uint64)
    n = data_off.size - 1
    if n < 0:
        raise ValueError(f"{what} data_off: needs n + 1 entries")
    mss = np.ascontiguousarray(mss, np.uint32)
    if mss.size < n:
        raise ValueError(f"{what} mss: {mss.size} entries for {n} super-segments")
    return data_off, mss, n


def tso_count_host(data_off: np.ndarray, mss: np.ndarray) -> np.ndarray:
    """nsx_tso_count_host: frame_first (n + 1), the prefix sum of max(1, ceil(len_s / mss_s)); frame_first[n] is the
    batch's frame count."""
    data_off, mss, n = _tso_host_args(data_off, mss, "tso_count_host")
    first = np.zeros(n + 1, np.uint64)
    _check(lib().nsx_tso_count_host(_np_ptr(data_off), _np_ptr(mss), n, _np_ptr(first)), "nsx_tso_count_host")
    return first


def tso_layout_host(data_off: np.ndarray, mss: np.ndarray, frame_first: np.ndarray,
                    opt_off: np.ndarray | None = None, ip_hdr_len: int = 20):
    """nsx_tso_layout_host: (frame_seg[n_frames], out_off[n_frames + 1]) — each frame's super-segment and the packed
    4-aligned frame slots of the expanded batch."""
    data_off, mss, n = _tso_host_args(data_off, mss, "tso_layout_host")
    first = np.ascontiguousarray(frame_first, np.uint64)
    if first.size < n + 1:
        raise ValueError(f"tso_layout_host frame_first: {first.size} entries for {n} super-segments")
    oo = None if opt_off is None else np.ascontiguousarray(opt_off, np.uint64)
    if oo is not None and oo.size < n + 1:
        raise ValueError(f"tso_layout_host opt_off: {oo.size} entries for {n} super-segments")
    # the C call checks frame_first against its own count before it writes: these sizes hold whenever it writes
    nf = int(first[n])
    if nf >= 1 << 40:
        raise ValueError(f"tso_layout_host frame_first: {nf} frames")
    seg = np.zeros(max(nf, 1), np.uint32)
    out = np.zeros(nf + 1, np.uint64)
    _check(lib().nsx_tso_layout_host(_np_ptr(oo), _np_ptr(data_off), _np_ptr(mss), _np_ptr(first), n, ip_hdr_len,
                                     _np_ptr(seg), _np_ptr(out)), "nsx_tso_layout_host")
    return seg[:nf], out


def _tso_build_dev(ipver: int, ip: dict, fields: dict, data, data_off, mss, frame_first, frame_seg, out, out_off, opts,
                   opt_off, raw, stream, tune, n_frames):
    what = f"tso_ipv{ipver}_tcp_build_dev"
    n = _count(data_off, f"{what} data_off")
    nf = _count(out_off, f"{what} out_off") if n_frames is None else int(n_frames)
    if nf < 0:
        raise ValueError(f"{what}: n_frames {nf}")
    _span(frame_seg, 4 * nf, f"{what} frame_seg", elem=4)
    sizes = _ip_sizes(ipver)
    for k in ("src", "dst"):
        if ip.get(k) is None:
            raise ValueError(f"{what}: address array {k!r} missing")
    for k in IP_FIELDS:
        _span(ip.get(k), sizes[k] * n, f"{what} {k}", elem=None if k in ("src", "dst") else sizes[k])
    for k, size in BUILD_FIELDS:
        if fields.get(k) is None and k != "offset":  # only byte 12 may be computed on the device
            raise ValueError(f"{what}: header field {k!r} missing")
        _span(fields.get(k), size * n, f"{what} {k}", elem=size)
    _span(data, 0, f"{what} data")
    _span(mss, 4 * n, f"{what} mss", elem=4)
    _span(frame_first, 8 * (n + 1), f"{what} frame_first", elem=8)
    _span(out_off, 8 * (nf + 1), f"{what} out_off", elem=8)
    if nf and (n <= 0 or nf < n):
        raise ValueError(f"{what}: {nf} frames for {n} super-segments")
    # the frame lengths are in device memory; the least a frame can take is an IP and a TCP header
    _span(out, nf * (40 if ipver == 4 else 60), f"{what} out", elem=1)
    _span(opt_off, 8 * (n + 1), f"{what} opt_off", elem=8)
    if opt_off is not None and opts is None:
        raise ValueError(f"{what}: opt_off given without opts")
    _span(opts, 0, f"{what} opts")
    _span(raw, 2 * nf, f"{what} raw", elem=2)
    ipsoa = IpHdrSoA(*[_dev_ptr(ip.get(k)) for k in IP_FIELDS])
    soa = TcpHdrSoA(*[_dev_ptr(fields.get(k)) for k, _ in BUILD_FIELDS])
    fn = getattr(lib(), f"nsx_tso_ipv{ipver}_tcp_build_dev_tuned")
    _check(fn(ctypes.byref(ipsoa), ctypes.byref(soa), _dev_ptr(opts), _dev_ptr(opt_off), _dev_ptr(data),
              _dev_ptr(data_off), data.numel(), _dev_ptr(mss), max(n, 0), _dev_ptr(frame_first), _dev_ptr(frame_seg),
              nf, _dev_ptr(out), _dev_ptr(out_off), _dev_ptr(raw), _stream(stream), _tune(tune)), f"nsx_{what}")
    return out


def tso_ipv4_tcp_build_dev(ip: dict, fields: dict, data, data_off, mss, frame_first, frame_seg, out, out_off,
                           opts=None, opt_off=None, raw=None, stream=None, tune=None, n_frames=None):
    """Segmentation offload on the transmit pass: ip, fields, opt_off, data_off and mss (uint32: payload bytes per
    frame) hold one entry per super-segment; frame_first / frame_seg / out_off are the frame map of tso_count_host
    and tso_layout_host as device tensors (frame_seg: one 4-byte entry per frame; out_off: one more — n_frames
    defaults to its length less one). Frame j of a super-segment carries seq + j·mss, FIN / PSH only when last, CWR only when
    first, ident + j. raw (optional): one TCP raw sum per frame."""
    return _tso_build_dev(4, ip, fields, data, data_off, mss, frame_first, frame_seg, out, out_off, opts, opt_off, raw,
                          stream, tune, n_frames)


def tso_ipv6_tcp_build_dev(ip: dict, fields: dict, data, data_off, mss, frame_first, frame_seg, out, out_off,
                           opts=None, opt_off=None, raw=None, stream=None, tune=None, n_frames=None):
    """The same for IPv6 (flow label and traffic class copied to every frame)."""
    return _tso_build_dev(6, ip, fields, data, data_off, mss, frame_first, frame_seg, out, out_off, opts, opt_off, raw,
                          stream, tune, n_frames)


def _tso_build_host(ipver: int, ip: dict, fields: dict, data, data_off, mss, frame_first, frame_seg, out_off, opts,
                    opt_off, out, want_raw, num_gpus, tune):
    what = f"tso_ipv{ipver}_tcp_build_host"
    data = np.ascontiguousarray(data, np.uint8)
    data_off, mss, n = _tso_host_args(data_off, mss, what)
    sizes = _ip_sizes(ipver)
    ipc = {}
    for k in IP_FIELDS:
        v = ip.get(k)
        if v is None:
            if k in ("src", "dst"):
                raise ValueError(f"{what}: address array {k!r} missing")
            continue
        v = np.ascontiguousarray(v, _IP_NP[k])
        if v.nbytes < sizes[k] * n:
            raise ValueError(f"{what} {k}: {v.nbytes} B given, {sizes[k] * n} B needed")
        ipc[k] = v
    cols = {}
    for k, _ in BUILD_FIELDS:
        v = fields.get(k)
        if v is None:
            if k != "offset":
                raise ValueError(f"{what}: header field {k!r} missing")
            continue
        v = np.ascontiguousarray(v, _BUILD_NP[k])
        if v.size < n:
            raise ValueError(f"{what} {k}: {v.size} entries for {n} super-segments")
        cols[k] = v
    oo = None if opt_off is None else np.ascontiguousarray(opt_off, np.uint64)
    if oo is not None and opts is None:
        raise ValueError(f"{what}: opt_off given without opts")
    if oo is not None and oo.size < n + 1:
        raise ValueError(f"{what} opt_off: {oo.size} entries for {n} super-segments")
    ob = None if opts is None else (np.ascontiguousarray(opts, np.uint8) if len(opts) else np.zeros(1, np.uint8))
    if frame_first is None:
        frame_first = tso_count_host(data_off, mss)
    first = np.ascontiguousarray(frame_first, np.uint64)
    if first.size < n + 1:
        raise ValueError(f"{what} frame_first: {first.size} entries for {n} super-segments")
    if frame_seg is None or out_off is None:
        seg0, off0 = tso_layout_host(data_off, mss, first, oo, 20 if ipver == 4 else 40)
        frame_seg = seg0 if frame_seg is None else frame_seg
        out_off = off0 if out_off is None else out_off
    seg = np.ascontiguousarray(frame_seg, np.uint32)
    out_off = np.ascontiguousarray(out_off, np.uint64)
    nf = int(first[n]) if n >= 0 else 0
    if seg.size < nf:
        raise ValueError(f"{what} frame_seg: {seg.size} entries for {nf} frames")
    if out_off.size < nf + 1:
        raise ValueError(f"{what} out_off: {out_off.size} entries for {nf} frames")
    if n > 0 and data.size < int(data_off[n]):
        raise ValueError(f"{what} data: {data.size} B given, data_off ends at {int(data_off[n])}")
    if oo is not None and n > 0 and ob.size < int(oo[n]):
        raise ValueError(f"{what} opts: {ob.size} B given, opt_off ends at {int(oo[n])}")
    if out is None:
        out = np.zeros(int(out_off[nf]), np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous:
        raise ValueError(f"{what} out: needs a C-contiguous uint8 array")
    if out.size < int(out_off[nf]):
        raise ValueError(f"{what} out: {out.size} B given, out_off ends at {int(out_off[nf])}")
    raw = np.empty(nf, np.uint16) if want_raw else None
    ipsoa = IpHdrSoA(*[_np_ptr(ipc.get(k)) for k in IP_FIELDS])
    soa = TcpHdrSoA(*[_np_ptr(cols.get(k)) for k, _ in BUILD_FIELDS])
    fn = getattr(lib(), f"nsx_tso_ipv{ipver}_tcp_build_host_tuned")
    _check(fn(ctypes.byref(ipsoa), ctypes.byref(soa), _np_ptr(ob), _np_ptr(oo), _np_ptr(data), _np_ptr(data_off),
              _np_ptr(mss), n, _np_ptr(first), _np_ptr(seg), nf, _np_ptr(out), _np_ptr(out_off), _np_ptr(raw), num_gpus,
              _tune(tune)), f"nsx_{what}")
    return out, raw


def tso_ipv4_tcp_build_host(ip: dict, fields: dict, data: np.ndarray, data_off: np.ndarray, mss: np.ndarray,
                            frame_first: np.ndarray | None = None, frame_seg: np.ndarray | None = None,
                            out_off: np.ndarray | None = None, opts: np.ndarray | None = None,
                            opt_off: np.ndarray | None = None, out: np.ndarray | None = None, want_raw: bool = True,
                            num_gpus: int = 0, tune=None):
    """Segmentation offload over host-resident super-segments (nsx_tso_ipv4_tcp_build_host): host arrays, one entry
    per super-segment; the frame map defaults to tso_count_host / tso_layout_host. Returns (out, raw or None), raw
    holding one sum per frame."""
    return _tso_build_host(4, ip, fields, data, data_off, mss, frame_first, frame_seg, out_off, opts, opt_off, out,
                           want_raw, num_gpus, tune)


def tso_ipv6_tcp_build_host(ip: dict, fields: dict, data: np.ndarray, data_off: np.ndarray, mss: np.ndarray,
                            frame_first: np.ndarray | None = None, frame_seg: np.ndarray | None = None,
                            out_off: np.ndarray | None = None, opts: np.ndarray | None = None,
                            opt_off: np.ndarray | None = None, out: np.ndarray | None = None, want_raw: bool = True,
                            num_gpus: int = 0, tune=None):
    return _tso_build_host(6, ip, fields, data, data_off, mss, frame_first, frame_seg, out_off, opts, opt_off, out,
                           want_raw, num_gpus, tune)


# ---------------------------------------------------------------------------
# receive coalescing: frames in, super-segments in segmentation offload's format out (nsx_gro_*)
# ---------------------------------------------------------------------------
# nsx_gro_out members in order: (name, torch dtype, worst-case element count as a function of (n, alen, buf bytes))
GRO_FIELDS = (("n_super", "int64", lambda n, a, b: 1),
              ("src", "uint8", lambda n, a, b: n * a), ("dst", "uint8", lambda n, a, b: n * a),
              ("ident", "int16", lambda n, a, b: n), ("ttl", "uint8", lambda n, a, b: n),
              ("tclass", "uint8", lambda n, a, b: n), ("flow", "int32", lambda n, a, b: n),
              ("src_port", "int16", lambda n, a, b: n), ("dst_port", "int16", lambda n, a, b: n),
              ("seq_num", "int32", lambda n, a, b: n), ("ack_num", "int32", lambda n, a, b: n),
              ("offset", "uint8", lambda n, a, b: n), ("control", "uint8", lambda n, a, b: n),
              ("window", "int16", lambda n, a, b: n), ("urgent_ptr", "int16", lambda n, a, b: n),
              ("mss", "int32", lambda n, a, b: n), ("opts", "uint8", lambda n, a, b: 40 * n),
              ("opt_off", "int64", lambda n, a, b: n + 1), ("data", "uint8", lambda n, a, b: b),
              ("data_off", "int64", lambda n, a, b: n + 1), ("first_frame", "int64", lambda n, a, b: n),
              ("frame_cnt", "int32", lambda n, a, b: n), ("frame_seg", "int32", lambda n, a, b: n))


class GroOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in GRO_FIELDS]


def gro_work_bytes(n: int) -> int:
    """nsx_gro_work_bytes: the scratch bytes one gro_ipv4_tcp_dev / gro_ipv6_tcp_dev call over n frames needs."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_gro_work_bytes(n, ctypes.byref(c)), "nsx_gro_work_bytes")
    return c.value


def gro_flow_work_bytes(n: int) -> int:
    """nsx_gro_flow_work_bytes: the scratch bytes one gro_flow_ipv4_tcp_dev / gro_flow_ipv6_tcp_dev call over n frames
    needs (at least gro_work_bytes(n))."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_gro_flow_work_bytes(n, ctypes.byref(c)), "nsx_gro_flow_work_bytes")
    return c.value


def _gro_dev(ipver: int, buf, offsets, valid, out, work, stream, tune, flow: bool = False, order=None) -> dict:
    import torch
    what = f"gro_flow_ipv{ipver}_tcp_dev" if flow else f"gro_ipv{ipver}_tcp_dev"
    n = _count(offsets, f"{what} offsets")
    alen = _ip_sizes(ipver)["src"]
    _span(buf, 0, f"{what} buf", elem=1)
    _span(valid, 8 * ((n + 63) // 64), f"{what} valid", elem=8)
    if valid is None:
        raise ValueError(f"{what}: the receive pass's mask `valid` is required")
    res = dict(out or {})
    bad = set(res) - {k for k, _, _ in GRO_FIELDS}
    if bad:
        raise ValueError(f"{what}: unknown output(s) {sorted(bad)}")
    for k, dt, count in GRO_FIELDS:
        need = count(n, alen, buf.numel())
        if res.get(k) is None:  # worst-case size; never a zero-size tensor, whose address is NULL
            res[k] = torch.empty(max(need, 1), dtype=getattr(torch, dt), device=offsets.device)
        size = np.dtype(dt).itemsize
        _span(res[k], need * size, f"{what} {k}", elem=size)
    if flow:
        if order is None:  # never a zero-size tensor, whose address is NULL
            order = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
        _span(order, 4 * n, f"{what} order", elem=4)
    need = gro_flow_work_bytes(n) if flow else gro_work_bytes(n)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=offsets.device)
    _span(work, need, f"{what} work")
    soa = GroOut(*[_dev_ptr(res[k]) for k, _, _ in GRO_FIELDS])
    fn = getattr(lib(), f"nsx_{what}_tuned")
    args = [_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(valid)] + ([_dev_ptr(order)] if flow else []) + \
        [ctypes.byref(soa), _dev_ptr(work), work.numel() * work.element_size(), _stream(stream), _tune(tune)]
    _check(fn(*args), f"nsx_{what}")
    if flow:
        res["order"] = order
    return res


def gro_ipv4_tcp_dev(buf, offsets, valid, out=None, work=None, stream=None, tune=None) -> dict:
    """TCP receive coalescing over packed IPv4/TCP frames: buf / offsets as rx_ipv4_tcp_verify_dev, valid = that
    pass's mask. Returns a dict of device tensors, the members of nsx_gro_out (GRO_FIELDS) — n_super (one int64),
    the per-super-segment arrays tso_ipv4_tcp_build_dev takes, first_frame / frame_cnt, and frame_seg per frame —
    allocated at worst-case size (n entries, n + 1 offsets, buf.numel() data bytes, 40·n option bytes) unless given
    in `out`; `work` is scratch of gro_work_bytes(n) bytes. Does not synchronise: n_super is in device memory."""
    return _gro_dev(4, buf, offsets, valid, out, work, stream, tune)


def gro_ipv6_tcp_dev(buf, offsets, valid, out=None, work=None, stream=None, tune=None) -> dict:
    """The same for IPv6 (src / dst 16 bytes per super-segment; ident 0; tclass and flow from the header)."""
    return _gro_dev(6, buf, offsets, valid, out, work, stream, tune)


def gro_flow_ipv4_tcp_dev(buf, offsets, valid, out=None, order=None, work=None, stream=None, tune=None) -> dict:
    """Flow-keyed receive coalescing over packed IPv4/TCP frames (nsx_gro_flow_ipv4_tcp_dev): gro_ipv4_tcp_dev per
    connection, however the connections interleave in the batch. Returns the GRO_FIELDS dict plus "order" (n int32:
    the stable sort of the frame indices by flow key, allocated unless given). first_frame holds positions in
    `order`, frame_seg stays indexed by the original frame. `work` is scratch of gro_flow_work_bytes(n) bytes;
    tune: run_segs and blocks_per_cu as gro_ipv4_tcp_dev, rows = keys per sort tile in units of 256."""
    return _gro_dev(4, buf, offsets, valid, out, work, stream, tune, flow=True, order=order)


def gro_flow_ipv6_tcp_dev(buf, offsets, valid, out=None, order=None, work=None, stream=None, tune=None) -> dict:
    """The same for IPv6."""
    return _gro_dev(6, buf, offsets, valid, out, work, stream, tune, flow=True, order=order)


# ---------------------------------------------------------------------------
# in-place NAT rewrite with incremental checksum update (nsx_nat_*)
# ---------------------------------------------------------------------------
NAT_TUPLE_BYTES = {4: 12, 6: 36}  # src, dst, the two ports, as on the wire
NAT_ENTRY_BYTES = {4: 32, 6: 80}  # match tuple, state dword, new tuple, zero dword


def nat_table_slots(n_rules: int) -> int:
    """nsx_nat_table_slots: the smallest power of two >= max(16, 2 * n_rules)."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_nat_table_slots(n_rules, ctypes.byref(c)), "nsx_nat_table_slots")
    return c.value


def nat_table_build_host(ip_ver: int, match: np.ndarray, new: np.ndarray, slots: int | None = None) -> np.ndarray:
    """nsx_nat_table_build_host: `match` and `new` are (n_rules, 12) (IPv4) or (n_rules, 36) (IPv6) uint8 tuples;
    returns the table, slots * 32 or slots * 80 bytes of host memory (slots defaults to nat_table_slots(n_rules)),
    for the caller to copy to the device."""
    if ip_ver not in NAT_TUPLE_BYTES:
        raise ValueError(f"nat_table_build_host: ip_ver must be 4 or 6, got {ip_ver}")
    tb = NAT_TUPLE_BYTES[ip_ver]
    match, new = np.ascontiguousarray(match, np.uint8), np.ascontiguousarray(new, np.uint8)
    if match.size % tb or match.size != new.size:
        raise ValueError(f"nat_table_build_host: match and new must hold the same number of {tb}-byte tuples, got "
                         f"{match.size} B and {new.size} B")
    n_rules = match.size // tb
    if slots is None:
        slots = nat_table_slots(n_rules)
    if not 0 <= slots <= 1 << 31:  # refused by the C call too; checked here before the table is allocated
        raise NsxError(NSX_EINVAL, "nsx_nat_table_build_host")
    table = np.empty(max(slots * NAT_ENTRY_BYTES[ip_ver], 1), np.uint8)
    _check(lib().nsx_nat_table_build_host(ip_ver, _np_ptr(match), _np_ptr(new), n_rules, _np_ptr(table), slots),
           "nsx_nat_table_build_host")
    return table[:slots * NAT_ENTRY_BYTES[ip_ver]]


def _nat_rewrite_dev(ipver: int, buf, offsets, valid, table, slots: int, ttl_dec: int, hit, stream):
    import torch
    what = f"nat_ipv{ipver}_tcp_rewrite_dev"
    n = _count(offsets, f"{what} offsets")
    words = (n + 63) // 64
    _span(buf, 0, f"{what} buf", elem=1)
    if valid is None:
        raise ValueError(f"{what}: the receive pass's mask `valid` is required")
    _span(valid, 8 * words, f"{what} valid", elem=8)
    if table is None:
        raise ValueError(f"{what}: `table` is required")
    if slots < 0 or slots > 1 << 31:
        raise ValueError(f"{what}: slots must be a power of two <= 2^31, got {slots}")
    _span(table, slots * NAT_ENTRY_BYTES[ipver], f"{what} table")
    if hit is None:  # never a zero-size tensor, whose address is NULL
        hit = torch.empty(max(words, 1), dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(hit, 8 * words, f"{what} hit", elem=8)
    if not 0 <= ttl_dec < 1 << 32:  # what a uint32_t can carry; the C call refuses 256 and up (NSX_EINVAL)
        raise ValueError(f"{what}: ttl_dec must be 0..255, got {ttl_dec}")
    fn = getattr(lib(), f"nsx_{what}")
    _check(fn(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(valid), _dev_ptr(table), slots, ttl_dec, _dev_ptr(hit),
              _stream(stream)), f"nsx_{what}")
    return hit


def nat_ipv4_tcp_rewrite_dev(buf, offsets, valid, table, slots: int, ttl_dec: int = 0, hit=None, stream=None):
    """In-place NAT rewrite over packed IPv4/TCP frames (nsx_nat_ipv4_tcp_rewrite_dev): buf / offsets as
    rx_ipv4_tcp_verify_dev, valid = that pass's mask, table = nat_table_build_host's bytes on the device (slots
    entries). Frames whose address / port tuple hits the table get the new tuple, TTL - ttl_dec and incrementally
    updated checksums, in `buf` itself. Returns `hit`: bit i%64 of hit[i//64] iff frame i was translated (int64
    words, allocated unless given). Does not synchronise."""
    return _nat_rewrite_dev(4, buf, offsets, valid, table, slots, ttl_dec, hit, stream)


def nat_ipv6_tcp_rewrite_dev(buf, offsets, valid, table, slots: int, ttl_dec: int = 0, hit=None, stream=None):
    """The same for IPv6 (36-byte tuples, 80-byte entries; the hop limit is covered by no checksum)."""
    return _nat_rewrite_dev(6, buf, offsets, valid, table, slots, ttl_dec, hit, stream)


# ---------------------------------------------------------------------------
# UDP: fused transmit pass, segmentation offload and receive verify (nsx_udp_*)
# ---------------------------------------------------------------------------
UDP_NO_CSUM = 1  # NSX_UDP_NO_CSUM
UDP_FIELDS = ("src_port", "dst_port")  # nsx_udp_hdr_soa members, 2-byte elements


class UdpHdrSoA(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in UDP_FIELDS]


def udp_layout_host(data_off: np.ndarray, ip_hdr_len: int = 20) -> np.ndarray:
    """nsx_udp_layout_host: packed 4-aligned frame offsets, out_off[i] = Σ_{j<i} round_up4(ip_hdr_len + 8 + len_j)."""
    data_off = np.ascontiguousarray(data_off, np.uint64)
    n = data_off.size - 1
    if n < 0:
        raise ValueError("udp_layout_host data_off: needs n + 1 entries")
    out = np.zeros(n + 1, np.uint64)
    _check(lib().nsx_udp_layout_host(_np_ptr(data_off), n, ip_hdr_len, _np_ptr(out)), "nsx_udp_layout_host")
    return out


def udp_uso_layout_host(data_off: np.ndarray, gso: np.ndarray, frame_first: np.ndarray, ip_hdr_len: int = 20):
    """nsx_udp_uso_layout_host: (frame_seg[n_frames], out_off[n_frames + 1]) over tso_count_host's frame map."""
    data_off, gso, n = _tso_host_args(data_off, gso, "udp_uso_layout_host")
    first = np.ascontiguousarray(frame_first, np.uint64)
    if first.size < n + 1:
        raise ValueError(f"udp_uso_layout_host frame_first: {first.size} entries for {n} super-datagrams")
    # the C call checks frame_first against its own count before it writes: these sizes hold whenever it writes
    nf = int(first[n])
    if nf >= 1 << 40:
        raise ValueError(f"udp_uso_layout_host frame_first: {nf} frames")
    seg = np.zeros(max(nf, 1), np.uint32)
    out = np.zeros(nf + 1, np.uint64)
    _check(lib().nsx_udp_uso_layout_host(_np_ptr(data_off), _np_ptr(gso), _np_ptr(first), n, ip_hdr_len, _np_ptr(seg),
                                         _np_ptr(out)), "nsx_udp_uso_layout_host")
    return seg[:nf], out


def _udp_soa(what: str, ipver: int, ip: dict, ports: dict, n: int):
    sizes = _ip_sizes(ipver)
    for k in ("src", "dst"):
        if ip.get(k) is None:
            raise ValueError(f"{what}: address array {k!r} missing")
    for k in IP_FIELDS:
        _span(ip.get(k), sizes[k] * n, f"{what} {k}", elem=None if k in ("src", "dst") else sizes[k])
    for k in UDP_FIELDS:
        if ports.get(k) is None:
            raise ValueError(f"{what}: header field {k!r} missing")
        _span(ports.get(k), 2 * n, f"{what} {k}", elem=2)


def _udp_tx_build_dev(ipver: int, ip: dict, ports: dict, data, data_off, out, out_off, flags, raw, stream, tune):
    what = f"udp_tx_ipv{ipver}_build_dev"
    n = _count(data_off, f"{what} data_off")
    _udp_soa(what, ipver, ip, ports, n)
    _span(data, 0, f"{what} data")
    _span(out_off, 8 * (n + 1), f"{what} out_off", elem=8)
    # the frame lengths are in device memory; the least n frames can take is an IP and a UDP header each
    _span(out, max(n, 0) * (28 if ipver == 4 else 48), f"{what} out", elem=1)
    _span(raw, 2 * n, f"{what} raw", elem=2)
    ipsoa = IpHdrSoA(*[_dev_ptr(ip.get(k)) for k in IP_FIELDS])
    soa = UdpHdrSoA(*[_dev_ptr(ports.get(k)) for k in UDP_FIELDS])
    fn = getattr(lib(), f"nsx_udp_tx_ipv{ipver}_build_dev_tuned")
    _check(fn(ctypes.byref(ipsoa), ctypes.byref(soa), _dev_ptr(data), _dev_ptr(data_off), data.numel(), n, int(flags),
              _dev_ptr(out), _dev_ptr(out_off), _dev_ptr(raw), _stream(stream), _tune(tune)), f"nsx_{what}")
    return out


def udp_tx_ipv4_build_dev(ip: dict, ports: dict, data, data_off, out, out_off, flags: int = 0, raw=None, stream=None,
                          tune=None):
    """UDP transmit pass: whole IPv4 datagrams carrying UDP (header checksum and UDP checksum in place) at out +
    out_off[i]. ip as tx_ipv4_tcp_build_dev; ports: dict of device tensors src_port, dst_port (2 B per frame);
    flags: UDP_NO_CSUM stores the field 0; raw (optional) receives the UDP raw sums."""
    return _udp_tx_build_dev(4, ip, ports, data, data_off, out, out_off, flags, raw, stream, tune)


def udp_tx_ipv6_build_dev(ip: dict, ports: dict, data, data_off, out, out_off, flags: int = 0, raw=None, stream=None,
                          tune=None):
    """The same for IPv6 (no flag is valid there)."""
    return _udp_tx_build_dev(6, ip, ports, data, data_off, out, out_off, flags, raw, stream, tune)


def _udp_uso_build_dev(ipver: int, ip: dict, ports: dict, data, data_off, gso, frame_first, frame_seg, out, out_off,
                       flags, raw, stream, tune, n_frames):
    what = f"udp_uso_ipv{ipver}_build_dev"
    n = _count(data_off, f"{what} data_off")
    nf = _count(out_off, f"{what} out_off") if n_frames is None else int(n_frames)
    if nf < 0:
        raise ValueError(f"{what}: n_frames {nf}")
    _span(frame_seg, 4 * nf, f"{what} frame_seg", elem=4)
    _udp_soa(what, ipver, ip, ports, n)
    _span(data, 0, f"{what} data")
    _span(gso, 4 * n, f"{what} gso", elem=4)
    _span(frame_first, 8 * (n + 1), f"{what} frame_first", elem=8)
    _span(out_off, 8 * (nf + 1), f"{what} out_off", elem=8)
    if nf and (n <= 0 or nf < n):
        raise ValueError(f"{what}: {nf} frames for {n} super-datagrams")
    _span(out, nf * (28 if ipver == 4 else 48), f"{what} out", elem=1)
    _span(raw, 2 * nf, f"{what} raw", elem=2)
    ipsoa = IpHdrSoA(*[_dev_ptr(ip.get(k)) for k in IP_FIELDS])
    soa = UdpHdrSoA(*[_dev_ptr(ports.get(k)) for k in UDP_FIELDS])
    fn = getattr(lib(), f"nsx_udp_uso_ipv{ipver}_build_dev_tuned")
    _check(fn(ctypes.byref(ipsoa), ctypes.byref(soa), _dev_ptr(data), _dev_ptr(data_off), data.numel(), _dev_ptr(gso),
              max(n, 0), _dev_ptr(frame_first), _dev_ptr(frame_seg), nf, int(flags), _dev_ptr(out), _dev_ptr(out_off),
              _dev_ptr(raw), _stream(stream), _tune(tune)), f"nsx_{what}")
    return out


def udp_uso_ipv4_build_dev(ip: dict, ports: dict, data, data_off, gso, frame_first, frame_seg, out, out_off,
                           flags: int = 0, raw=None, stream=None, tune=None, n_frames=None):
    """UDP segmentation offload: ip, ports, data_off and gso (uint32: payload bytes per datagram) hold one entry per
    super-datagram; frame_first / frame_seg / out_off are the frame map of tso_count_host and udp_uso_layout_host as
    device tensors (n_frames defaults to out_off's length less one). Frame j carries ident + j."""
    return _udp_uso_build_dev(4, ip, ports, data, data_off, gso, frame_first, frame_seg, out, out_off, flags, raw,
                              stream, tune, n_frames)


def udp_uso_ipv6_build_dev(ip: dict, ports: dict, data, data_off, gso, frame_first, frame_seg, out, out_off,
                           flags: int = 0, raw=None, stream=None, tune=None, n_frames=None):
    """The same for IPv6."""
    return _udp_uso_build_dev(6, ip, ports, data, data_off, gso, frame_first, frame_seg, out, out_off, flags, raw,
                              stream, tune, n_frames)


def udp_rx_ipv4_verify_dev(buf, offsets, mask=None, ip_raw=None, udp_raw=None, stream=None, tune=None):
    """UDP receive verify over packed IPv4/UDP frames: validity bitmask (+ optional raw sums)."""
    import torch
    n = _count(offsets, "udp_rx_ipv4_verify_dev offsets")
    if mask is None:
        mask = torch.empty((max(n, 0) + 63) // 64, dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(buf, 0, "udp_rx_ipv4_verify_dev buf")
    _span(mask, 8 * ((n + 63) // 64), "udp_rx_ipv4_verify_dev mask", elem=8)
    _span(ip_raw, 2 * n, "udp_rx_ipv4_verify_dev ip_raw", elem=2)
    _span(udp_raw, 2 * n, "udp_rx_ipv4_verify_dev udp_raw", elem=2)
    _check(lib().nsx_udp_rx_ipv4_verify_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(mask),
                                                  _dev_ptr(ip_raw), _dev_ptr(udp_raw), _stream(stream), _tune(tune)),
           "nsx_udp_rx_ipv4_verify_dev")
    return mask


def udp_rx_ipv6_verify_dev(buf, offsets, mask=None, udp_raw=None, stream=None, tune=None):
    """UDP receive verify over packed IPv6/UDP packets: validity bitmask (+ optional raw sums)."""
    import torch
    n = _count(offsets, "udp_rx_ipv6_verify_dev offsets")
    if mask is None:
        mask = torch.empty((max(n, 0) + 63) // 64, dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(buf, 0, "udp_rx_ipv6_verify_dev buf")
    _span(mask, 8 * ((n + 63) // 64), "udp_rx_ipv6_verify_dev mask", elem=8)
    _span(udp_raw, 2 * n, "udp_rx_ipv6_verify_dev udp_raw", elem=2)
    _check(lib().nsx_udp_rx_ipv6_verify_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(mask),
                                                  _dev_ptr(udp_raw), _stream(stream), _tune(tune)),
           "nsx_udp_rx_ipv6_verify_dev")
    return mask


# ---------------------------------------------------------------------------
# UDP receive coalescing: datagrams in, super-datagrams in UDP segmentation offload's format out (nsx_ugro_*)
# ---------------------------------------------------------------------------
# nsx_ugro_out members in order: (name, torch dtype, worst-case element count as a function of (n, alen, buf bytes))
UGRO_FIELDS = (("n_super", "int64", lambda n, a, b: 1),
               ("src", "uint8", lambda n, a, b: n * a), ("dst", "uint8", lambda n, a, b: n * a),
               ("ident", "int16", lambda n, a, b: n), ("ttl", "uint8", lambda n, a, b: n),
               ("tclass", "uint8", lambda n, a, b: n), ("flow", "int32", lambda n, a, b: n),
               ("src_port", "int16", lambda n, a, b: n), ("dst_port", "int16", lambda n, a, b: n),
               ("gso", "int32", lambda n, a, b: n), ("data", "uint8", lambda n, a, b: b),
               ("data_off", "int64", lambda n, a, b: n + 1), ("first_frame", "int64", lambda n, a, b: n),
               ("frame_cnt", "int32", lambda n, a, b: n), ("frame_seg", "int32", lambda n, a, b: n))


class UgroOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in UGRO_FIELDS]


def ugro_work_bytes(n: int) -> int:
    """nsx_ugro_work_bytes: the scratch bytes one ugro_ipv4_dev / ugro_ipv6_dev call over n frames needs."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_ugro_work_bytes(n, ctypes.byref(c)), "nsx_ugro_work_bytes")
    return c.value


def ugro_flow_work_bytes(n: int) -> int:
    """nsx_ugro_flow_work_bytes: the scratch bytes one ugro_flow_ipv4_dev / ugro_flow_ipv6_dev call over n frames
    needs (at least ugro_work_bytes(n))."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_ugro_flow_work_bytes(n, ctypes.byref(c)), "nsx_ugro_flow_work_bytes")
    return c.value


def _ugro_dev(ipver: int, buf, offsets, valid, out, work, stream, tune, flow: bool = False, order=None) -> dict:
    import torch
    what = f"ugro_flow_ipv{ipver}_dev" if flow else f"ugro_ipv{ipver}_dev"
    n = _count(offsets, f"{what} offsets")
    alen = _ip_sizes(ipver)["src"]
    _span(buf, 0, f"{what} buf", elem=1)
    _span(valid, 8 * ((n + 63) // 64), f"{what} valid", elem=8)
    if valid is None:
        raise ValueError(f"{what}: the UDP receive verify's mask `valid` is required")
    res = dict(out or {})
    bad = set(res) - {k for k, _, _ in UGRO_FIELDS}
    if bad:
        raise ValueError(f"{what}: unknown output(s) {sorted(bad)}")
    for k, dt, count in UGRO_FIELDS:
        need = count(n, alen, buf.numel())
        if res.get(k) is None:  # worst-case size; never a zero-size tensor, whose address is NULL
            res[k] = torch.empty(max(need, 1), dtype=getattr(torch, dt), device=offsets.device)
        size = np.dtype(dt).itemsize
        _span(res[k], need * size, f"{what} {k}", elem=size)
    if flow:
        if order is None:  # never a zero-size tensor, whose address is NULL
            order = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
        _span(order, 4 * n, f"{what} order", elem=4)
    need = ugro_flow_work_bytes(n) if flow else ugro_work_bytes(n)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=offsets.device)
    _span(work, need, f"{what} work")
    soa = UgroOut(*[_dev_ptr(res[k]) for k, _, _ in UGRO_FIELDS])
    fn = getattr(lib(), f"nsx_{what}_tuned")
    args = [_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(valid)] + ([_dev_ptr(order)] if flow else []) + \
        [ctypes.byref(soa), _dev_ptr(work), work.numel() * work.element_size(), _stream(stream), _tune(tune)]
    _check(fn(*args), f"nsx_{what}")
    if flow:
        res["order"] = order
    return res


def ugro_ipv4_dev(buf, offsets, valid, out=None, work=None, stream=None, tune=None) -> dict:
    """UDP receive coalescing over packed IPv4/UDP frames: buf / offsets as udp_rx_ipv4_verify_dev, valid = that
    pass's mask. Returns a dict of device tensors, the members of nsx_ugro_out (UGRO_FIELDS) — n_super (one int64),
    the per-super-datagram arrays udp_uso_ipv4_build_dev takes, first_frame / frame_cnt, and frame_seg per frame —
    allocated at worst-case size (n entries, n + 1 offsets, buf.numel() data bytes) unless given in `out`; `work` is
    scratch of ugro_work_bytes(n) bytes; tune: run_segs = frames per scan block, blocks_per_cu = the copy kernel's
    grid. Does not synchronise: n_super is in device memory."""
    return _ugro_dev(4, buf, offsets, valid, out, work, stream, tune)


def ugro_ipv6_dev(buf, offsets, valid, out=None, work=None, stream=None, tune=None) -> dict:
    """The same for IPv6 (src / dst 16 bytes per super-datagram; ident 0; tclass and flow from the header)."""
    return _ugro_dev(6, buf, offsets, valid, out, work, stream, tune)


def ugro_flow_ipv4_dev(buf, offsets, valid, out=None, order=None, work=None, stream=None, tune=None) -> dict:
    """Flow-keyed UDP receive coalescing (nsx_ugro_flow_ipv4_dev): ugro_ipv4_dev per flow, however the flows
    interleave in the batch. Returns the UGRO_FIELDS dict plus "order" (n int32: the stable sort of the frame indices
    by flow key, allocated unless given). first_frame holds positions in `order`, frame_seg stays indexed by the
    original frame. `work` is scratch of ugro_flow_work_bytes(n) bytes; tune: as ugro_ipv4_dev, and rows = keys per
    sort tile in units of 256."""
    return _ugro_dev(4, buf, offsets, valid, out, work, stream, tune, flow=True, order=order)


def ugro_flow_ipv6_dev(buf, offsets, valid, out=None, order=None, work=None, stream=None, tune=None) -> dict:
    """The same for IPv6."""
    return _ugro_dev(6, buf, offsets, valid, out, work, stream, tune, flow=True, order=order)


# ---------------------------------------------------------------------------
# IPv4 fragmentation and reassembly (nsx_frag_*, nsx_reasm_*)
# ---------------------------------------------------------------------------
FRAG_PASS, FRAG_CUT, FRAG_DF, FRAG_BAD = 0, 1, 2, 3
# nsx_reasm_out members in order: (name, torch dtype, worst-case element count as a function of (n, buf bytes))
REASM_FIELDS = (("n_out", "int64", lambda n, b: 1), ("out", "uint8", lambda n, b: b),
                ("out_off", "int64", lambda n, b: n + 1), ("first_pos", "int64", lambda n, b: n),
                ("frag_cnt", "int32", lambda n, b: n), ("frame_seg", "int32", lambda n, b: n),
                ("is_frag", "int64", lambda n, b: (n + 63) // 64))


class ReasmOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in REASM_FIELDS]


def _frag_host_args(offsets, mtu, what: str):
    offsets = np.ascontiguousarray(offsets, np.uint64)
    mtu = np.ascontiguousarray(mtu, np.uint32)
    n = offsets.size - 1
    if n < 0 or mtu.size < n:
        raise ValueError(f"{what}: offsets needs n + 1 entries and mtu n, got {offsets.size} and {mtu.size}")
    return offsets, mtu, n


def frag_count_host(offsets: np.ndarray, mtu: np.ndarray) -> np.ndarray:
    """nsx_frag_count_host: frag_first (n + 1), the prefix sum of the output slots each frame takes at its mtu."""
    offsets, mtu, n = _frag_host_args(offsets, mtu, "frag_count_host")
    first = np.zeros(n + 1, np.uint64)
    _check(lib().nsx_frag_count_host(_np_ptr(offsets), _np_ptr(mtu), n, _np_ptr(first)), "nsx_frag_count_host")
    return first


def frag_layout_host(offsets: np.ndarray, mtu: np.ndarray, frag_first: np.ndarray):
    """nsx_frag_layout_host: (frag_src[n_frags], out_off[n_frags + 1]) over frag_count_host's map; dense slots."""
    offsets, mtu, n = _frag_host_args(offsets, mtu, "frag_layout_host")
    first = np.ascontiguousarray(frag_first, np.uint64)
    if first.size < n + 1:
        raise ValueError(f"frag_layout_host frag_first: {first.size} entries for {n} frames")
    # the C call checks frag_first against its own count before it writes: these sizes hold whenever it writes
    nf = int(first[n])
    if nf >= 1 << 40:
        raise ValueError(f"frag_layout_host frag_first: {nf} slots")
    src = np.zeros(max(nf, 1), np.uint32)
    out = np.zeros(nf + 1, np.uint64)
    _check(lib().nsx_frag_layout_host(_np_ptr(offsets), _np_ptr(mtu), _np_ptr(first), n, _np_ptr(src), _np_ptr(out)),
           "nsx_frag_layout_host")
    return src[:nf], out


def frag_ipv4_dev(buf, offsets, mtu, frag_first, frag_src, out, out_off, status=None, stream=None, tune=None,
                  n_frags=None):
    """IPv4 fragmentation over packed frames: buf / offsets as the receive passes take them, mtu (uint32 per frame),
    and the frame map of frag_count_host / frag_layout_host as device tensors (n_frags defaults to out_off's length
    less one). Writes the slots to out + out_off[t] and returns status (uint8 per frame: FRAG_PASS, FRAG_CUT, FRAG_DF,
    FRAG_BAD; allocated unless given). The slot extents are in device memory: `out` must hold out_off[n_frags] bytes.
    tune: blocks_per_cu = the grid."""
    import torch
    what = "frag_ipv4_dev"
    n = _count(offsets, f"{what} offsets")
    nf = _count(out_off, f"{what} out_off") if n_frags is None else int(n_frags)
    if nf < n or (n == 0 and nf):
        raise ValueError(f"{what}: {nf} slots for {n} frames")
    if status is None:  # never a zero-size tensor, whose address is NULL
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=offsets.device)
    _span(buf, 0, f"{what} buf", elem=1)
    _span(mtu, 4 * n, f"{what} mtu", elem=4)
    _span(frag_first, 8 * (n + 1), f"{what} frag_first", elem=8)
    _span(frag_src, 4 * nf, f"{what} frag_src", elem=4)
    _span(out_off, 8 * (nf + 1), f"{what} out_off", elem=8)
    _span(out, 0, f"{what} out", elem=1)
    _span(status, n, f"{what} status", elem=1)
    _check(lib().nsx_frag_ipv4_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), _dev_ptr(mtu), n, _dev_ptr(frag_first),
                                         _dev_ptr(frag_src), nf, _dev_ptr(out), _dev_ptr(out_off), _dev_ptr(status),
                                         _stream(stream), _tune(tune)), f"nsx_{what}")
    return status


def reasm_work_bytes(n: int) -> int:
    """nsx_reasm_work_bytes: the scratch bytes one reasm_ipv4_dev call over n frames needs."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_reasm_work_bytes(n, ctypes.byref(c)), "nsx_reasm_work_bytes")
    return c.value


def reasm_ipv4_dev(buf, offsets, out=None, order=None, work=None, stream=None, tune=None) -> dict:
    """IPv4 reassembly over packed frames: returns a dict of device tensors, the members of nsx_reasm_out
    (REASM_FIELDS) — n_out (one int64), the datagrams in out / out_off, first_pos / frag_cnt per datagram, frame_seg
    per frame, the member bitmask is_frag — allocated at worst-case size (n entries, n + 1 offsets, buf.numel() output
    bytes) unless given in `out`, plus "order" (n int32, allocated unless given). `work` is scratch of
    reasm_work_bytes(n) bytes; tune: run_segs = frames per scan block, blocks_per_cu = the copy kernel's grid, rows =
    keys per sort tile in units of 256. Does not synchronise: n_out is in device memory."""
    import torch
    what = "reasm_ipv4_dev"
    n = _count(offsets, f"{what} offsets")
    _span(buf, 0, f"{what} buf", elem=1)
    res = dict(out or {})
    bad = set(res) - {k for k, _, _ in REASM_FIELDS}
    if bad:
        raise ValueError(f"{what}: unknown output(s) {sorted(bad)}")
    for k, dt, count in REASM_FIELDS:
        need = count(n, buf.numel())
        if res.get(k) is None:  # worst-case size; never a zero-size tensor, whose address is NULL
            res[k] = torch.empty(max(need, 1), dtype=getattr(torch, dt), device=offsets.device)
        size = np.dtype(dt).itemsize
        _span(res[k], need * size, f"{what} {k}", elem=size)
    if order is None:  # never a zero-size tensor, whose address is NULL
        order = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
    _span(order, 4 * n, f"{what} order", elem=4)
    need = reasm_work_bytes(n)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=offsets.device)
    _span(work, need, f"{what} work")
    soa = ReasmOut(*[_dev_ptr(res[k]) for k, _, _ in REASM_FIELDS])
    _check(lib().nsx_reasm_ipv4_dev_tuned(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(order), ctypes.byref(soa),
                                          _dev_ptr(work), work.numel() * work.element_size(), _stream(stream),
                                          _tune(tune)), f"nsx_{what}")
    res["order"] = order
    return res


# ---------------------------------------------------------------------------
# ICMP: error generation, request helpers, receive verify and the in-place echo reply (nsx_icmp_*)
# ---------------------------------------------------------------------------
ICMP_NONE, ICMP_SENT, ICMP_QUIET, ICMP_BAD, ICMP_LIMITED = 0, 1, 2, 3, 4
ICMP_HDR = {4: 28, 6: 48}       # IP header + ICMP header of a generated message
ICMP_QUOTE = {4: 548, 6: 1232}  # the most bytes of the offending frame a message quotes
# nsx_icmp_err_out members in order: (name, torch dtype, worst-case element count as a function of (n, m, out bytes)),
# m = min(n, max_out) the most messages
ICMP_ERR_FIELDS = (("n_out", "int64", lambda n, m, b: 1), ("out", "uint8", lambda n, m, b: b),
                   ("out_off", "int64", lambda n, m, b: m + 1), ("src_frame", "int32", lambda n, m, b: m),
                   ("status", "uint8", lambda n, m, b: n))


class IcmpErrCfg(ctypes.Structure):
    _fields_ = [("src", ctypes.c_uint8 * 16), ("ttl", ctypes.c_uint32), ("ident0", ctypes.c_uint32),
                ("max_out", ctypes.c_uint64)]


class IcmpErrOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in ICMP_ERR_FIELDS]


def icmp_err_work_bytes(n: int) -> int:
    """nsx_icmp_err_work_bytes: the scratch bytes one icmp_err_ipv4_dev / icmp_err_ipv6_dev call over n frames needs."""
    c = ctypes.c_uint64(0)
    _check(lib().nsx_icmp_err_work_bytes(n, ctypes.byref(c)), "nsx_icmp_err_work_bytes")
    return c.value


def icmp_err_out_bytes(ipver: int, n: int, max_out: int, buf_bytes: int) -> int:
    """The worst-case bytes of `out`: min(n, max_out) messages of a full quote each, and never more than the batch's
    own bytes plus a header per message."""
    m = min(n, max_out)
    return min(m * (ICMP_HDR[ipver] + ICMP_QUOTE[ipver]), buf_bytes + m * ICMP_HDR[ipver])


def _icmp_err_dev(ipver: int, buf, offsets, req, arg, src, ttl, ident0, max_out, out, work, stream, tune) -> dict:
    import torch
    what = f"icmp_err_ipv{ipver}_dev"
    n = _count(offsets, f"{what} offsets")
    max_out = n if max_out is None else int(max_out)
    src = bytes(src)
    if len(src) != (4 if ipver == 4 else 16):
        raise ValueError(f"{what}: src must be {4 if ipver == 4 else 16} address bytes, got {len(src)}")
    if not 0 <= ttl < 1 << 32 or not 0 <= ident0 < 1 << 32 or not 0 <= max_out < 1 << 64:
        raise ValueError(f"{what}: ttl, ident0 and max_out must be unsigned, got {ttl}, {ident0}, {max_out}")
    _span(buf, 0, f"{what} buf", elem=1)
    if req is None:
        raise ValueError(f"{what}: the request words `req` are required")
    _span(req, 4 * n, f"{what} req", elem=4)
    _span(arg, 4 * n, f"{what} arg", elem=4)
    res = dict(out or {})
    bad = set(res) - {k for k, _, _ in ICMP_ERR_FIELDS}
    if bad:
        raise ValueError(f"{what}: unknown output(s) {sorted(bad)}")
    m = min(n, max_out)
    ob = icmp_err_out_bytes(ipver, n, max_out, buf.numel())
    for k, dt, count in ICMP_ERR_FIELDS:
        need = count(n, m, ob)
        if res.get(k) is None:  # worst-case size; never a zero-size tensor, whose address is NULL
            res[k] = torch.empty(max(need, 1), dtype=getattr(torch, dt), device=offsets.device)
        size = np.dtype(dt).itemsize
        # the bytes of `out` are data-dependent (out_off is in device memory): a caller's own tensor is taken as given
        _span(res[k], 0 if k == "out" and out and out.get("out") is not None else need * size, f"{what} {k}", elem=size)
    need = icmp_err_work_bytes(n)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=offsets.device)
    _span(work, need, f"{what} work")
    cfg = IcmpErrCfg((ctypes.c_uint8 * 16)(*src), ttl, ident0, max_out)
    soa = IcmpErrOut(*[_dev_ptr(res[k]) for k, _, _ in ICMP_ERR_FIELDS])
    fn = getattr(lib(), f"nsx_{what}_tuned")
    _check(fn(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(req), _dev_ptr(arg), ctypes.byref(cfg), ctypes.byref(soa),
              _dev_ptr(work), work.numel() * work.element_size(), _stream(stream), _tune(tune)), f"nsx_{what}")
    return res


def icmp_err_ipv4_dev(buf, offsets, req, src, arg=None, ttl: int = 64, ident0: int = 0, max_out: int | None = None,
                      out=None, work=None, stream=None, tune=None) -> dict:
    """ICMP error generation over packed IPv4 frames (nsx_icmp_err_ipv4_dev): buf / offsets as the receive passes take
    them, req one request word per frame (0 none, else type | code << 8; int32), arg the word for ICMP header bytes
    4-7 (None: all zero), src our own 4 address bytes, max_out the most messages (default n). Returns a dict of device
    tensors, the members of nsx_icmp_err_out (ICMP_ERR_FIELDS) — n_out (one int64), the messages in out / out_off,
    src_frame per message, status per frame (ICMP_NONE, ICMP_SENT, ICMP_QUIET, ICMP_BAD, ICMP_LIMITED) — allocated at
    worst-case size (icmp_err_out_bytes) unless given in `out`. `work` is scratch of icmp_err_work_bytes(n) bytes;
    tune: run_segs = frames per scan block, blocks_per_cu = the emit kernel's grid. Does not synchronise."""
    return _icmp_err_dev(4, buf, offsets, req, arg, src, ttl, ident0, max_out, out, work, stream, tune)


def icmp_err_ipv6_dev(buf, offsets, req, src, arg=None, ttl: int = 64, ident0: int = 0, max_out: int | None = None,
                      out=None, work=None, stream=None, tune=None) -> dict:
    """The same for IPv6 (16 address bytes, ICMPv6 types 1-4, quotes of up to 1232 bytes; ident0 is unused)."""
    return _icmp_err_dev(6, buf, offsets, req, arg, src, ttl, ident0, max_out, out, work, stream, tune)


def icmp_req_frag_dev(status, mtu, req, arg, stream=None):
    """nsx_icmp_req_frag_dev: where status[i] == FRAG_DF (frag_ipv4_dev's status), req[i] = 3 | 4 << 8 and arg[i] =
    mtu[i] & 0xFFFF; every other entry of req / arg (int32, n each) stays as it was. Returns (req, arg)."""
    what = "icmp_req_frag_dev"
    if status is None or mtu is None or req is None or arg is None:
        raise ValueError(f"{what}: status, mtu, req and arg are required")
    _span(req, 0, f"{what} req", elem=4)
    n = req.numel()
    _span(status, n, f"{what} status", elem=1)
    _span(mtu, 4 * n, f"{what} mtu", elem=4)
    _span(arg, 4 * n, f"{what} arg", elem=4)
    _check(lib().nsx_icmp_req_frag_dev(_dev_ptr(status), _dev_ptr(mtu), n, _dev_ptr(req), _dev_ptr(arg),
                                       _stream(stream)), f"nsx_{what}")
    return req, arg


def _icmp_req_ttl_dev(ipver: int, buf, offsets, valid, ttl_dec: int, req, arg, stream):
    what = f"icmp_req_ttl_ipv{ipver}_dev"
    n = _count(offsets, f"{what} offsets")
    _span(buf, 0, f"{what} buf", elem=1)
    if valid is None or req is None or arg is None:
        raise ValueError(f"{what}: `valid`, `req` and `arg` are required")
    _span(valid, 8 * ((n + 63) // 64), f"{what} valid", elem=8)
    _span(req, 4 * n, f"{what} req", elem=4)
    _span(arg, 4 * n, f"{what} arg", elem=4)
    if not 0 <= ttl_dec < 1 << 32:  # what a uint32_t can carry; the C call refuses 256 and up (NSX_EINVAL)
        raise ValueError(f"{what}: ttl_dec must be 0..255, got {ttl_dec}")
    fn = getattr(lib(), f"nsx_{what}")
    _check(fn(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(valid), ttl_dec, _dev_ptr(req), _dev_ptr(arg),
              _stream(stream)), f"nsx_{what}")
    return req, arg


def icmp_req_ttl_ipv4_dev(buf, offsets, valid, ttl_dec: int, req, arg, stream=None):
    """nsx_icmp_req_ttl_ipv4_dev: where frame i's valid bit is set, it holds a whole IPv4 header and its TTL is <=
    ttl_dec (the frames the NAT rewrite refuses on TTL), req[i] = 11 and arg[i] = 0. Returns (req, arg)."""
    return _icmp_req_ttl_dev(4, buf, offsets, valid, ttl_dec, req, arg, stream)


def icmp_req_ttl_ipv6_dev(buf, offsets, valid, ttl_dec: int, req, arg, stream=None):
    """The same for IPv6: the hop limit, req[i] = 3."""
    return _icmp_req_ttl_dev(6, buf, offsets, valid, ttl_dec, req, arg, stream)


def _icmp_rx_verify_dev(ipver: int, buf, offsets, mask, ip_raw, icmp_raw, type, stream, tune):
    import torch
    what = f"icmp_rx_ipv{ipver}_verify_dev"
    n = _count(offsets, f"{what} offsets")
    if mask is None:  # never a zero-size tensor, whose address is NULL
        mask = torch.empty(max((n + 63) // 64, 1), dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(buf, 0, f"{what} buf")
    _span(mask, 8 * ((n + 63) // 64), f"{what} mask", elem=8)
    _span(ip_raw, 2 * n, f"{what} ip_raw", elem=2)
    _span(icmp_raw, 2 * n, f"{what} icmp_raw", elem=2)
    _span(type, 2 * n, f"{what} type", elem=2)
    fn = getattr(lib(), f"nsx_{what}_tuned")
    raws = (_dev_ptr(ip_raw), _dev_ptr(icmp_raw)) if ipver == 4 else (_dev_ptr(icmp_raw),)
    _check(fn(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(mask), *raws, _dev_ptr(type), _stream(stream),
              _tune(tune)), f"nsx_{what}")
    return mask


def icmp_rx_ipv4_verify_dev(buf, offsets, mask=None, ip_raw=None, icmp_raw=None, type=None, stream=None, tune=None):
    """ICMP receive verify over packed IPv4 frames: validity bitmask (+ optional raw sums, and type << 8 | code per
    frame — 0xFFFF unless the bit is set — in `type`, int16)."""
    return _icmp_rx_verify_dev(4, buf, offsets, mask, ip_raw, icmp_raw, type, stream, tune)


def icmp_rx_ipv6_verify_dev(buf, offsets, mask=None, icmp_raw=None, type=None, stream=None, tune=None):
    """ICMPv6 receive verify over packed IPv6 packets: validity bitmask (+ optional raw sum and type << 8 | code)."""
    return _icmp_rx_verify_dev(6, buf, offsets, mask, None, icmp_raw, type, stream, tune)


def _icmp_echo_reply_dev(ipver: int, buf, offsets, valid, ttl: int, hit, stream):
    import torch
    what = f"icmp_echo_reply_ipv{ipver}_dev"
    n = _count(offsets, f"{what} offsets")
    words = (n + 63) // 64
    _span(buf, 0, f"{what} buf", elem=1)
    if valid is None:
        raise ValueError(f"{what}: the verify's mask `valid` is required")
    _span(valid, 8 * words, f"{what} valid", elem=8)
    if hit is None:  # never a zero-size tensor, whose address is NULL
        hit = torch.empty(max(words, 1), dtype=torch.int64, device=offsets.device)  # u64 bits
    _span(hit, 8 * words, f"{what} hit", elem=8)
    if not 0 <= ttl < 1 << 32:  # what a uint32_t can carry; the C call refuses 256 and up (NSX_EINVAL)
        raise ValueError(f"{what}: ttl must be 0..255, got {ttl}")
    fn = getattr(lib(), f"nsx_{what}")
    _check(fn(_dev_ptr(buf), _dev_ptr(offsets), n, _dev_ptr(valid), ttl, _dev_ptr(hit), _stream(stream)),
           f"nsx_{what}")
    return hit


def icmp_echo_reply_ipv4_dev(buf, offsets, valid, ttl: int = 64, hit=None, stream=None):
    """In-place echo reply over packed IPv4 frames (nsx_icmp_echo_reply_ipv4_dev): valid = icmp_rx_ipv4_verify_dev's
    mask. Echo requests to a unicast address become their replies in `buf` itself: addresses swapped, TTL = ttl, type
    0, both checksums updated incrementally. Returns `hit`: bit i%64 of hit[i//64] iff frame i was answered (int64
    words, allocated unless given). Does not synchronise."""
    return _icmp_echo_reply_dev(4, buf, offsets, valid, ttl, hit, stream)


def icmp_echo_reply_ipv6_dev(buf, offsets, valid, ttl: int = 64, hit=None, stream=None):
    """The same for IPv6 (type 128 becomes 129; the hop limit is covered by no checksum)."""
    return _icmp_echo_reply_dev(6, buf, offsets, valid, ttl, hit, stream)


def fill_splitmix64_dev(buf, seed: int, byte_off: int = 0, stream=None):
    _span(buf, 0, "fill_splitmix64_dev buf")
    _check(lib().nsx_fill_splitmix64_dev(_dev_ptr(buf), byte_off, buf.numel() * buf.element_size(), seed,
                                         _stream(stream)), "nsx_fill_splitmix64_dev")
    return buf
