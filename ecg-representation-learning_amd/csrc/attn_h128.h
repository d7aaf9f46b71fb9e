// Launchers of the dh = 128 attention kernels (attention_h128.hip), called by the entry points in attention.hip once they have checked the
// arguments.  Library-internal: hidden, not part of the C-ABI.
#pragma once
#include <cstdint>

#define ECGVIT_H128_API __attribute__((visibility("hidden")))
ECGVIT_H128_API int attn_h128_fwd(const void *qkv, void *out, float *lse, int B, int N, int h, float scale, uint64_t seed, uint32_t th, float ik,
                                  void *stream);
ECGVIT_H128_API int attn_h128_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, int B, int N, int h, float scale,
                                  uint64_t seed, uint32_t th, float ik, void *stream);
ECGVIT_H128_API int attn_h128_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, int B, int N, int h, float scale, uint64_t seed, uint32_t th,
                                      float ik, void *stream);
ECGVIT_H128_API int attn_h128_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls, int B,
                                      int N, int h, float scale, uint64_t seed, uint32_t th, float ik, void *stream);
