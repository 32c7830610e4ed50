// The W register kind of trace programs (nx_trace_program; NX_T_PACK32 .. NX_T_REMU32 of include/nexus_hip.h): a register holding a raw
// 32-bit integer that need not be canonical — the RV32M chips' 64-bit product bytes and quotients (reference
// prover/src/chips/instructions/m/).  What air_jit.hip needs of it, in one place: which opcodes read and write the kind, the validation
// messages, the cost estimate that feeds "air.segment", the prelude text and the statement of every opcode.
//
// A register has the kind its latest writer gave it (the program is straight-line, so the kind at an instruction is static).  The
// generated kernels keep every register in a u32, so a W value is that u32 as it is; the segment cutter's backward slices recompute a W
// value in every kernel whose stores need it, as they do for any other value.
#pragma once
#include <string>
#include "../../include/nexus_hip.h"

namespace nx {

inline bool is_w_opcode(uint32_t op) { return op >= NX_T_PACK32 && op <= NX_T_REMU32; }
inline bool w_opcode_reads_w(uint32_t op) { return is_w_opcode(op) && op != NX_T_PACK32; }                         // PACK32 reads two canonical words
inline bool w_opcode_writes_w(uint32_t op) { return is_w_opcode(op) && op != NX_T_LO16 && op != NX_T_HI16; }       // LO16 / HI16 give canonical words
inline bool w_opcode_is_unary(uint32_t op) { return op == NX_T_LO16 || op == NX_T_HI16; }
inline bool uses_w_opcodes(const nx_cinstr* prog, uint32_t n_instr) { for (uint32_t i = 0; i < n_instr; i++) if (is_w_opcode(prog[i].op)) return true; return false; }

// why instruction `op` must not read a register of this kind, or nullptr
inline const char* w_kind_error(uint32_t op, bool reg_is_w) {
    if (w_opcode_reads_w(op) && !reg_is_w) return "an operand register of a 32-bit integer opcode does not hold a 32-bit integer (PACK32 makes one)";
    if (!w_opcode_reads_w(op) && reg_is_w) return "a 32-bit integer register read by a field opcode (LO16 / HI16 give its halves)";
    return nullptr;
}

// rough gfx950 instruction counts: the products are quarter-rate; the division is one reciprocal sequence (v_cvt_f32_u32, v_rcp_iflag_f32,
// three v_mul_hi_u32, fix-ups) and the zero-divisor select
inline uint32_t w_instr_cost(uint32_t op) {
    switch (op) {
    case NX_T_PACK32: return 2; case NX_T_LO16: case NX_T_HI16: return 1; case NX_T_MULLO32: return 2; case NX_T_MULHU32: return 4;
    default: return 40;
    }
}

// Part of the text only of a program that uses one of these opcodes: every other program generates the source it always did.  RISC-V's
// rules make the division total, so there is still no error path at run time.
static const char* const TRACE_W_PRELUDE = R"SRC(
FI u32 t_mulhu32(u32 a, u32 b) { return (u32)(((u64)a * b) >> 32); }
FI u32 t_divu32(u32 a, u32 b) { return b ? a / b : 0xffffffffu; }
FI u32 t_remu32(u32 a, u32 b) { return b ? a % b : a; }
)SRC";

inline std::string trace_w_statement(const nx_cinstr& in) {
    auto R = [](uint32_t i) { return "r" + std::to_string(i); };
    const std::string lhs = "  " + R(in.dst) + " = ";
    switch (in.op) {
    case NX_T_PACK32: return lhs + R(in.a) + " + (" + R(in.b) + " << 16);\n";
    case NX_T_LO16: return lhs + R(in.a) + " & 0xffffu;\n";
    case NX_T_HI16: return lhs + R(in.a) + " >> 16;\n";
    case NX_T_MULLO32: return lhs + R(in.a) + " * " + R(in.b) + ";\n";
    case NX_T_MULHU32: return lhs + "t_mulhu32(" + R(in.a) + ", " + R(in.b) + ");\n";
    case NX_T_DIVU32: return lhs + "t_divu32(" + R(in.a) + ", " + R(in.b) + ");\n";
    case NX_T_REMU32: return lhs + "t_remu32(" + R(in.a) + ", " + R(in.b) + ");\n";
    default: return std::string();
    }
}

}  // namespace nx
