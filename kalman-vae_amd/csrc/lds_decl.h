// lds_decl.h — how a kernel declares an LDS array:  KV_LDS(float, name, [ROWS][COLS]);  KV_LDS16(...) for one read as float4;
// KV_LDS_DYN(float, name) for the dynamic LDS of the launch.
// On the GPU this is the plain `__shared__` declaration.  In the test-only emulated workgroups (tests/hostsim/wave_emu.h,
// KVAE_WAVE_EMU) the array is a per-workgroup heap object of exactly its size, so that AddressSanitizer sees its bounds.
// KV_LDS_RD(arr, i): a read whose index may be far outside the allocation ON PURPOSE (the zero padding of csrc/vae_conv_mid.h:
// a DS read past the end of LDS returns 0).  On the GPU it is exactly (arr)[i]; emulated, an index inside the workgroup's LDS
// object is the real read, one at 1 << 24 elements or above is 0.f, anything between aborts (wemu::lds_read).
#pragma once

#if !defined(KVAE_WAVE_EMU)
#define KV_LDS(T, name, dims) __shared__ T name dims
#define KV_LDS16(T, name, dims) __shared__ __attribute__((aligned(16))) T name dims
#define KV_LDS_DYN(T, name) extern __shared__ T name[]
#define KV_LDS_RD(arr, i) (arr)[i]
#else
#define KV_LDS_AT(T, name, dims, key) \
  typedef T name##_lds_t dims;        \
  name##_lds_t &name = *static_cast<name##_lds_t *>(wemu::block_shared((key), sizeof(name##_lds_t)))
#define KV_LDS(T, name, dims) KV_LDS_AT(T, name, dims, __COUNTER__)
#define KV_LDS16(T, name, dims) KV_LDS_AT(T, name, dims, __COUNTER__)
#define KV_LDS_DYN(T, name) T *name = static_cast<T *>(wemu::block_dyn_shared())
#define KV_LDS_RD(arr, i) wemu::lds_read((arr), (i), #arr)
#endif
