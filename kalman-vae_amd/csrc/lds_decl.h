// lds_decl.h — how a kernel declares an LDS array:  KV_LDS(float, name, [ROWS][COLS]);  KV_LDS16(...) for one read as float4;
// KV_LDS_DYN(float, name) for the dynamic LDS of the launch.
// On the GPU this is the plain `__shared__` declaration.  In the test-only emulated workgroups (tests/hostsim/wave_emu.h,
// KVAE_WAVE_EMU) the array is a per-workgroup heap object of exactly its size, so that AddressSanitizer sees its bounds.
#pragma once

#if !defined(KVAE_WAVE_EMU)
#define KV_LDS(T, name, dims) __shared__ T name dims
#define KV_LDS16(T, name, dims) __shared__ __attribute__((aligned(16))) T name dims
#define KV_LDS_DYN(T, name) extern __shared__ T name[]
#else
#define KV_LDS_AT(T, name, dims, key) \
  typedef T name##_lds_t dims;        \
  name##_lds_t &name = *static_cast<name##_lds_t *>(wemu::block_shared((key), sizeof(name##_lds_t)))
#define KV_LDS(T, name, dims) KV_LDS_AT(T, name, dims, __COUNTER__)
#define KV_LDS16(T, name, dims) KV_LDS_AT(T, name, dims, __COUNTER__)
#define KV_LDS_DYN(T, name) T *name = static_cast<T *>(wemu::block_dyn_shared())
#endif
