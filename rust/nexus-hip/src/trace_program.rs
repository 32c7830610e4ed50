//! Derived trace columns filled on the device (`nx_trace_program`, include/nexus_hip.h): the row-local part of the reference's
//! `MachineChip::fill_main_trace` (prover/src/traits.rs:34-40) — AddChip's ValueA bytes and CarryFlag bits from ValueB / ValueC
//! (prover/src/chips/instructions/i/add.rs:26-96), SllChip's Rem / Qt / shift bits (sll.rs:33-111), the preprocessed is_first and
//! counter columns (prover/src/trace/preprocessed.rs:65-99) — recorded as a straight-line program over the base-field register file
//! and run once per row where the trace lives.  The host uploads the seed columns (the emulator's step values) and nothing else.
//!
//! ```ignore
//! let mut t = TraceProgram::new();
//! let (b, c) = (t.load(0, 0), t.load(1, 0));
//! let s = t.add(b, c);                                  // two bytes: the integer sum
//! let k255 = t.constant(255); let k8 = t.constant(8);
//! let lo = t.and(s, k255); t.store(2, lo);              // the ValueA byte
//! let carry = t.shr(s, k8); t.store(3, carry);          // the CarryFlag
//! session.trace_program(&t, &cols, log_size)?;          // cols: what tree_begin handed out
//! ```
//! The same operations as `ProgramBuilder` of nexus-zkvm_amd/air_program.py; every value takes a register of its own (the library
//! allows 4096), the instructions are emitted in the order they are recorded.
use crate::{try_check, HipError, Session};
use nexus_hip_sys as sys;

/// A value of the row program: the register that holds it.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Reg(u32);

#[derive(Default, Clone)]
pub struct TraceProgram {
    instrs: Vec<sys::nx_cinstr>,
    n_regs: u32,
    n_stores: usize,
}

impl TraceProgram {
    pub fn new() -> Self { Self::default() }
    fn push(&mut self, op: u32, a: u32, b: u32) -> Reg {
        let dst = self.n_regs;
        self.n_regs += 1;
        self.instrs.push(sys::nx_cinstr { op, dst, a, b });
        Reg(dst)
    }
    /// column `col` of the table at natural row `i + offset` (mod the trace length)
    pub fn load(&mut self, col: u32, offset: i32) -> Reg { self.push(sys::NX_C_LOAD, col, offset as u32) }
    /// a canonical M31 immediate (`v` < p)
    pub fn constant(&mut self, v: u32) -> Reg { self.push(sys::NX_C_CONST, v, 0) }
    /// the natural trace row (the VM step), not the storage position
    pub fn row(&mut self) -> Reg { self.push(sys::NX_T_ROW, 0, 0) }
    pub fn add(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_C_ADD, x.0, y.0) }
    pub fn sub(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_C_SUB, x.0, y.0) }
    pub fn mul(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_C_MUL, x.0, y.0) }
    pub fn neg(&mut self, x: Reg) -> Reg { self.push(sys::NX_C_NEG, x.0, 0) }
    /// bitwise on the canonical words as 32-bit integers; the result is written mod p
    pub fn and(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_AND, x.0, y.0) }
    pub fn or(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_OR, x.0, y.0) }
    pub fn xor(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_XOR, x.0, y.0) }
    /// `x << n` truncated to 32 bits, mod p; a count >= 32 gives 0
    pub fn shl(&mut self, x: Reg, n: Reg) -> Reg { self.push(sys::NX_T_SHL, x.0, n.0) }
    /// `x >> n`; a count >= 32 gives 0
    pub fn shr(&mut self, x: Reg, n: Reg) -> Reg { self.push(sys::NX_T_SHR, x.0, n.0) }
    /// 1 if x < y as integers, else 0
    pub fn ltu(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_LTU, x.0, y.0) }
    pub fn eq(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_EQ, x.0, y.0) }
    /// the M31 inverse; the inverse of 0 is 0 (is-zero helper columns)
    pub fn inv(&mut self, x: Reg) -> Reg { self.push(sys::NX_T_INV, x.0, 0) }
    /// a 32-bit integer register (the W kind) from a low and a high half-word: `(lo + (hi << 16))` truncated to 32 bits.  The five
    /// opcodes below work on such registers only; a field opcode or a store that reads one is refused
    pub fn pack32(&mut self, lo: Reg, hi: Reg) -> Reg { self.push(sys::NX_T_PACK32, lo.0, hi.0) }
    /// the low / high half-word of a 32-bit integer register, a canonical word again
    pub fn lo16(&mut self, w: Reg) -> Reg { self.push(sys::NX_T_LO16, w.0, 0) }
    pub fn hi16(&mut self, w: Reg) -> Reg { self.push(sys::NX_T_HI16, w.0, 0) }
    /// the low / high 32 bits of the unsigned 64-bit product
    pub fn mullo32(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_MULLO32, x.0, y.0) }
    pub fn mulhu32(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_MULHU32, x.0, y.0) }
    /// RISC-V DIVU / REMU: a zero divisor gives 0xFFFF_FFFF / the dividend
    pub fn divu32(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_DIVU32, x.0, y.0) }
    pub fn remu32(&mut self, x: Reg, y: Reg) -> Reg { self.push(sys::NX_T_REMU32, x.0, y.0) }
    /// `cols[col][row] = value`
    pub fn store(&mut self, col: u32, value: Reg) {
        self.instrs.push(sys::nx_cinstr { op: sys::NX_T_STORE, dst: 0, a: col, b: value.0 });
        self.n_stores += 1;
    }
    /// `cols[col][row] = value` on the rows where `flag` is not 0; the column keeps its content elsewhere (several chips share ValueA,
    /// each on the rows of its own opcode flag)
    pub fn store_if(&mut self, flag: Reg, col: u32, value: Reg) {
        self.instrs.push(sys::nx_cinstr { op: sys::NX_T_STORE_IF, dst: flag.0, a: col, b: value.0 });
        self.n_stores += 1;
    }
    pub fn instrs(&self) -> &[sys::nx_cinstr] { &self.instrs }
    pub fn n_regs(&self) -> u32 { self.n_regs.max(1) }
    pub fn n_stores(&self) -> usize { self.n_stores }
}

impl Session {
    /// Runs `program` once per row over `cols`: trace-domain evaluations of 2^log_size words in bit-reversed circle-domain order, what
    /// `tree_begin` handed out before the commit (null where the program touches nothing).  Stream-ordered: the commit, a check or a
    /// download that follows orders after it.  Refusals (a load of a stored column, a register read before it is written, a null or
    /// shared output column ...) are `HipError::Argument` with the instruction named.
    pub fn trace_program(&mut self, program: &TraceProgram, cols: &[*mut u32], log_size: u32) -> Result<(), HipError> {
        try_check(self.ctx, unsafe { sys::nx_trace_program(self.ctx, program.instrs.as_ptr(), program.instrs.len() as u32, program.n_regs(), cols.as_ptr(), cols.len() as u32, log_size, std::ptr::null_mut()) })
    }
}
