// kernels.hip.h -- the signature of every kernel runtime.hip launches, written once.  runtime.hip
// includes it to name the kernels, and every file that defines one of them includes it too, so
// the definition and the launch are checked against the same line (a return type, a template
// head or an attribute that differs is an error at the definition; parameters that differ still
// make an overload, which C++ allows, and show at link time as before).  Launch bounds and the
// per-file waves attributes stay on the definitions.  The column codecs' two kernel templates
// are declared in autopack.hip.h, in front of their bodies.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bitar_hip {
template <uint32_t RING, uint32_t HLOG>
__global__ void lz4_compress_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                    uint8_t* const*, uint32_t*, uint32_t*, const uint32_t*);
template <bool FARK>
__global__ void lz4_decompress_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                      const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                                      uint32_t*, unsigned long long*, const uint32_t*);
__global__ void snappy_compress_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                       uint8_t* const*, uint32_t*, const uint32_t*);
template <bool JOINED>
__global__ void snappy_decompress_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                         const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                                         uint32_t*, const uint32_t*);
__global__ void snappy_joined_key_kernel(const uint64_t*, uint32_t, uint32_t*);
__global__ void snappy_join_sizes_kernel(const uint32_t*, uint32_t, uint64_t, uint32_t*);
__global__ void snappy_join_kernel(const uint8_t*, uint64_t, const uint32_t*, uint64_t*, uint32_t,
                                   uint64_t, uint8_t*, uint64_t, uint64_t*, uint32_t*);
__global__ void snappy_scan_init_kernel(const uint8_t*, uint32_t, uint64_t, uint64_t*, uint32_t*,
                                        uint4*, uint32_t*, uint32_t);
__global__ void snappy_scan_walk_kernel(const uint8_t*, uint32_t, uint32_t, const uint32_t*, uint4*,
                                        uint2*, const uint2*);
__global__ void snappy_scan_resolve_kernel(const uint8_t*, uint32_t, uint64_t, uint64_t, uint32_t,
                                           uint32_t*, uint4*, const uint2*, uint4*, uint2*,
                                           uint64_t*, uint32_t*);
__global__ void snappy_scan_serial_kernel(const uint8_t*, uint32_t, uint64_t, uint64_t, uint32_t,
                                          uint32_t*, const uint4*, uint64_t*, uint32_t*, uint32_t);
__global__ void snappy_scan_finish_kernel(const uint8_t*, uint32_t, uint64_t, uint32_t,
                                          const uint32_t*, const uint4*, const uint4*, uint64_t*,
                                          uint32_t*);
__global__ void seg_cost_kernel(const uint8_t*, uint64_t, uint32_t, uint32_t, uint32_t*);
__global__ void order_hist_kernel(const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t,
                                  uint32_t*);
__global__ void order_scatter_kernel(const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t,
                                     uint32_t, const uint32_t*, uint32_t*, uint32_t, uint32_t);
__global__ void deflate_compress_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                        uint8_t* const*, uint32_t*, uint32_t*, const uint32_t*);
__global__ void deflate_compress_bits_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*,
                                             uint64_t, uint8_t* const*, uint32_t*, uint32_t*,
                                             const uint32_t*, uint32_t*);
__global__ void inflate_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                               const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                               uint32_t*, uint32_t, unsigned long long*, const uint32_t*);
__global__ void inflate_fixed_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                               const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                               uint32_t*, uint32_t, unsigned long long*, const uint32_t*);
template <uint32_t L>
__global__ void inflate_lanes_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                     const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*);
__global__ void zstd_parse_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t, uint2*, const uint32_t*);
__global__ void zstd_entropy_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                    const uint2*, uint8_t*, uint64_t, const uint32_t*);
__global__ void zstd_walk_kernel(const uint8_t*, uint64_t, uint32_t, uint32_t, uint8_t*, uint64_t,
                                 const uint32_t*);
__global__ void walk_key_kernel(const uint2*, uint32_t, uint32_t*);
__global__ void zstd_emit_kernel(const uint8_t*, uint64_t, uint32_t, const uint8_t*, uint64_t,
                                 uint8_t*, uint64_t, uint8_t* const*, uint32_t*, const uint8_t*,
                                 uint64_t, const uint32_t*);
__global__ void zstd_decompress_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                       const uint32_t*, uint32_t, uint32_t, uint8_t*,
                                       uint32_t*, uint32_t*, uint32_t, uint8_t*,
                                       unsigned long long*, const uint32_t*, uint32_t);
template <uint32_t S, uint32_t B>
__global__ void zstd_hlit_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                 const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                                 const uint8_t*, uint32_t*, const uint32_t*);
__global__ void hand_key_kernel(const uint32_t*, const uint8_t*, uint32_t, uint32_t, uint32_t*);
template <uint32_t L>
__global__ void zstd_handoff_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                    const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                                    const uint8_t*, uint32_t*);
template <uint32_t L, uint32_t B>
__global__ void zstd_seqdec_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                   const uint32_t*, uint32_t, uint32_t, uint32_t*, uint8_t*,
                                   uint64_t*, uint32_t, uint32_t*, unsigned long long*, const uint32_t*);
__global__ void zstd_exec_kernel(const uint8_t* const*, const uint8_t*, uint64_t, uint32_t,
                                 uint32_t, uint8_t*, uint32_t*, const uint8_t*,
                                 const uint64_t*, uint32_t, uint32_t*, unsigned long long*, const uint32_t*);
template <uint32_t L>
__global__ void zstd_lanes_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                  const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*);
__global__ void deflate_dyn_parse_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                         uint32_t*, const uint32_t*);
__global__ void deflate_dyn_emit_kernel(const uint8_t*, uint64_t, uint32_t, const uint8_t*,
                                        uint64_t, uint8_t*, uint64_t, uint8_t* const*, uint32_t*,
                                        uint32_t*, const uint32_t*, uint32_t*);
__global__ void join_scan_kernel(const uint8_t*, uint64_t, const uint32_t*, const uint32_t*,
                                 uint32_t, uint64_t, uint64_t*, uint32_t*);
__global__ void deflate_join_kernel(const uint8_t*, uint64_t, const uint32_t*, const uint32_t*,
                                    uint32_t, const uint64_t*, uint32_t*, uint64_t);
__global__ void deflate_split_kernel(const uint8_t*, uint64_t, const uint64_t*, const uint32_t*,
                                     uint32_t, uint8_t*, uint64_t, uint32_t*, uint32_t*);
__global__ void crc32_combine_kernel(const uint64_t*, uint64_t, uint32_t, uint32_t, uint32_t*);
__global__ void checksum_kernel(uint32_t, const uint8_t*, uint64_t, uint32_t, const uint32_t*,
                                uint32_t, uint64_t*);
template <uint32_t W, bool BITS, bool INV>
__global__ void filter_kernel(const uint8_t*, uint64_t, uint32_t, const uint32_t*, uint32_t,
                              uint8_t*);
__global__ void autopack_select_kernel(const uint8_t*, uint64_t, const uint32_t*, uint32_t, uint32_t,
                                       uint32_t, uint8_t*, uint64_t, uint8_t* const*, uint32_t*);
__global__ void autopack_route_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                      const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                                      uint32_t*);
__global__ void scan_sizes_kernel(const uint32_t*, uint32_t, uint64_t, uint64_t*, uint32_t*);
__global__ void pack_kernel(const uint8_t*, uint64_t, const uint32_t*, const uint64_t*, uint32_t,
                            uint8_t*);
__global__ void fill_kernel(int, uint64_t, uint64_t, uint8_t*, uint64_t);
__global__ void lz4_chain_kernel(const uint8_t*, uint32_t, const uint32_t*, uint32_t, uint8_t*,
                                 uint32_t, uint32_t*, uint32_t*);
__global__ void copy_batch_kernel(const uint8_t* const*, uint8_t* const*, const uint32_t*, uint32_t);
__global__ void lz4f_sizes_kernel(const uint32_t*, uint32_t, uint64_t, uint32_t, uint32_t*);
__global__ void lz4f_pack_kernel(const uint8_t*, uint64_t, uint32_t, const uint8_t*, uint64_t,
                                 const uint32_t*, const uint64_t*, uint32_t, uint8_t*);
}  // namespace bitar_hip
