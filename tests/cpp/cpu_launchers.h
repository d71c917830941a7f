// cpu_launchers.h — the plain C++ restatements behind the launcher stand-ins of cpu_launchers.cpp, callable on their
// own: tests/cpp/test_host_batch.cpp runs each once, synchronously, over the caller's whole arrays to get the bytes
// the chunked, sharded driver must reproduce.
//
// `st` is the stream a launcher queued the work on: every pointer must then lie in device memory of that stream's
// device (fake_hip.h). Null means ordinary memory: the contract's own assertions still run, the block checks do not.
// A broken contract ends the program with a message and a non-zero exit status.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../network-stack_amd/csrc/csum_kernels.h"

namespace ref {

// The raw one's-complement sum of include/nsx_csum.h over prefix ‖ bytes, the prefix given as its partial.
uint16_t csum(uint32_t partial, const uint8_t* p, uint64_t len);

void fixed(hipStream_t st, const uint8_t* base, uint64_t stride, uint32_t seg_len, uint64_t n, const uint32_t* partial,
           uint16_t* out);
void ragged(hipStream_t st, const uint8_t* base, const uint64_t* offsets, uint64_t n, const uint32_t* partial,
            uint16_t* out, uint8_t* ok);
void rx_tcp(hipStream_t st, int ipver, const uint8_t* base, const uint64_t* offsets, uint64_t n, uint64_t* mask);
void tcp_build(hipStream_t st, int ipver, const nsx::IpHdrSoA* ip, const nsx::TcpHdrSoA& h, const uint8_t* opts,
               const uint64_t* opt_off, const uint8_t* data, const uint64_t* data_off, uint64_t data_bytes,
               const uint32_t* partial, uint64_t n, uint8_t* out, const uint64_t* out_off, uint16_t* raw);
void tso_build(hipStream_t st, int ipver, const nsx::IpHdrSoA& ip, const nsx::TsoMap& tso, const nsx::TcpHdrSoA& h,
               const uint8_t* opts, const uint64_t* opt_off, const uint8_t* data, const uint64_t* data_off,
               uint64_t data_bytes, uint64_t n_frames, uint8_t* out, const uint64_t* out_off, uint16_t* raw);

}  // namespace ref
