// The device side of the stores both keccak trace kernels make (keccak_round.hip, keccak_memcheck.hip): every column leaves as
// single-word stores at the lane's byte offset through address space 1, with the column pointer read from the pointer table through the
// constant address space (the table is written before the launch and never by it), so that it is a scalar load and wave-uniform.
// Included inside namespace nx behind internal.h.
#define NX_KR_CONSTANT __attribute__((address_space(4)))

__device__ __forceinline__ u64 kr_gld64(const u64* p) { return *(NX_GLOBAL_AS const u64*)p; }
__device__ __forceinline__ void kr_gst64(u64* p, u64 v) { *(NX_GLOBAL_AS u64*)p = v; }

// cols: a table of column pointers in device memory; off: the byte offset of this lane's storage position (< 2^32: log_size <= 30)
typedef u32* KrColumn;
struct KrDevStore {
    NX_KR_CONSTANT const KrColumn* cols; u32 off;
    __device__ __forceinline__ void word(u32 col, u32 w) const { *(NX_GLOBAL_AS u32*)((NX_GLOBAL_AS char*)cols[col] + off) = w; }
    // The same store with the offset as a value this basic block defines.  A store takes the `global_store_dword v, v, s[ptr:ptr+1]` form
    // only where instruction selection sees column pointer + zext(off) in ONE block; across a loop that is not unrolled the extension is
    // hoisted, off arrives as a 64-bit pair and every store pays a v_lshl_add_u64 and a VGPR pair.  Emits nothing.
    __device__ __forceinline__ KrDevStore here() const { u32 o = off; asm volatile("" : "+v"(o)); return KrDevStore{cols, o}; }
    __device__ __forceinline__ void put(u32 col, u64 lane) const {
#pragma unroll
        for (u32 b = 0; b < 8; b++) word(col + b, (u32)(lane >> (8 * b)) & 255u);
    }
};
