// Natural coset row <-> storage position of a trace column (bit-reversed circle-domain order; reference
// prover/src/trace/utils_external.rs:24-39).  ONE text with two readers: the translation units that compile it (logup.hip,
// access_history.cuh) and air_jit.hip, which defines NX_TRACE_ROWS_AS_TEXT and takes it as a string literal into the preludes of the
// kernels hiprtc compiles (TRACE_ROWS_PRELUDE; FI is those preludes' own macro).  No preprocessor lines and no string literals inside
// the parentheses.  bitrev: field.cuh / AIR_PRELUDE.
#ifdef NX_TRACE_ROWS_AS_TEXT
#define NX_TRACE_ROWS_(...) #__VA_ARGS__
#else
#define NX_TRACE_ROWS_(...) __VA_ARGS__
#define FI NX_HD
#endif
NX_TRACE_ROWS_(
FI u32 pos_of_coset_row(u32 c, int log) { const u32 N = 1u << log; const u32 d = (c & 1) ? N - 1 - (c >> 1) : (c >> 1); return bitrev(d, log); }
FI u32 coset_row_of_pos(u32 p, int log) { const u32 N = 1u << log; const u32 d = bitrev(p, log); return d < N / 2 ? 2 * d : 2 * (N - 1 - d) + 1; }
)
#ifndef NX_TRACE_ROWS_AS_TEXT
#undef FI
#endif
#undef NX_TRACE_ROWS_
