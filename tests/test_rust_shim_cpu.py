"""The Rust binding under rust/ cannot be compiled here (no cargo / rustc in the image); what a compiler would catch about the FFI
surface is checked textually instead: the -sys crate is exactly what tools/gen_rust_sys.py generates from include/nexus_hip.h,
names and arities agree with an independent parse of the header, and the hand-written `nexus-hip` crate only calls functions the
-sys crate declares, with the declared number of arguments."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYS = os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")
HIP = os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")
HIP_DIR = os.path.join(ROOT, "rust", "nexus-hip")
HEADER = os.path.join(ROOT, "include", "nexus_hip.h")


def _split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "(<[{"
        depth -= ch in ")>]}"
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return out


def header_functions():
    t = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    t = re.sub(r"typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;", "", t, flags=re.S)   # callbacks inside nx_comm are fields, not functions
    fns = {}
    for m in re.finditer(r"\b(nx_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", t, flags=re.S):
        args = m.group(2).strip()
        fns[m.group(1)] = 0 if args in ("", "void") else len(_split_args(args))
    return fns


def rust_extern_functions():
    src = open(SYS).read()
    block = src[src.index('extern "C" {'):]
    return {m.group(1): (0 if not m.group(2).strip() else len(_split_args(m.group(2)))) for m in re.finditer(r"pub fn (nx_\w+)\((.*?)\)(?: -> [^;]+)?;", block)}


def test_sys_crate_is_what_the_generator_emits():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_every_header_function_is_bound_with_the_same_arity():
    h, r = header_functions(), rust_extern_functions()
    assert len(h) >= 80
    assert set(h) == set(r), (sorted(set(h) - set(r)), sorted(set(r) - set(h)))
    assert {k: v for k, v in h.items() if r[k] != v} == {}


def test_structs_mirror_the_header_field_for_field():
    src = open(SYS).read()
    t = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, n_fields in (("nx_component_spec", 6), ("nx_pcs_config", 7), ("nx_cinstr", 4), ("nx_air_component", 14), ("nx_comm", 11), ("nx_logup_frac", 6)):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, src, flags=re.S).group(1)
        assert len(re.findall(r"^\s*pub \w+:", body, flags=re.M)) == n_fields, name
    assert "log_constraint_degree_bound" in re.search(r"typedef struct nx_component_spec \{(.*?)\}", t, flags=re.S).group(1)


def _hand_written_sources():
    out = {}
    for d, _, fs in os.walk(HIP_DIR):
        for f in fs:
            if f.endswith(".rs"):
                out[os.path.relpath(os.path.join(d, f), ROOT)] = open(os.path.join(d, f)).read()
    return out


def test_hand_written_crate_calls_only_declared_functions_with_the_declared_arity():
    decl = rust_extern_functions()
    src = "\n".join(_hand_written_sources().values())
    calls = list(re.finditer(r"sys::(nx_\w+)\(", src))
    assert len(calls) > 50
    for m in calls:
        name = m.group(1)
        assert name in decl, name
        # the argument list: balanced parentheses from the call site
        i, depth = m.end(), 1
        while depth:
            depth += src[i] == "("
            depth -= src[i] == ")"
            i += 1
        args = src[m.end():i - 1].strip()
        n = 0 if not args else len(_split_args(args))
        assert n == decl[name], (name, n, decl[name])
    assert "core/src/lib.rs:22-24" in src


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference-side artefacts must be written against what the reference shows.  The reference checkout is not part
# of this repository: these tests hold our Rust to what was extracted from it into tests/golden/reference_*.txt, and re-derive those
# fixtures from the checkout as well when NX_REFERENCE_DIR names one.
REFERENCE = os.environ.get("NX_REFERENCE_DIR") or None


def _ref_src(rel):
    return open(os.path.join(REFERENCE, rel)).read()


def _load_scanner():
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_use_paths", os.path.join(ROOT, "tools", "reference_use_paths.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _observed():
    return set(open(os.path.join(ROOT, "tests", "golden", "reference_use_paths.txt")).read().split())


def _unobserved_listed():
    out = {}
    for line in open(os.path.join(ROOT, "rust", "UNOBSERVED_PATHS.txt")):
        line = line.strip()
        if line and not line.startswith("#"):
            parts = [x.strip() for x in line.split("|")]
            assert len(parts) == 3 and parts[1], "rust/UNOBSERVED_PATHS.txt: `path | why | what the reference shows` expected: " + line
            out[parts[0]] = parts[1]
    return out


def test_fixture_of_reference_paths_is_current():
    """tests/golden/reference_use_paths.txt is what tools/reference_use_paths.py extracts from the reference: one path per line, sorted,
    each under a root the scanner looks for, holding the facts the shim rests on (re-extracted and compared when NX_REFERENCE_DIR
    names a reference checkout)."""
    R = _load_scanner()
    lines = open(os.path.join(ROOT, "tests", "golden", "reference_use_paths.txt")).read().split()
    assert lines == sorted(set(lines)) and all(p.startswith(R.ROOTS) for p in lines)
    if REFERENCE:
        assert R.scan([REFERENCE]) == _observed()
    obs = _observed()
    # the facts the shim rests on: the pinned Stwo is the post-split crate
    for p in ("stwo::prover::backend::simd::SimdBackend", "stwo::prover::poly::circle::PolyOps", "stwo::prover::CommitmentSchemeProver", "stwo::core::proof::StarkProof",
              "stwo::core::vcs::blake2_merkle::Blake2sMerkleChannel", "stwo_constraint_framework::EvalAtRow", "nexus_vm::trace::k_trace_direct"):
        assert p in obs, p
    assert not any(p.startswith("stwo_prover::") for p in obs)


def test_every_stwo_and_nexus_path_in_our_rust_is_observed_in_the_reference_or_listed():
    """Every `stwo…` / `stwo_constraint_framework…` / `nexus_…` path named by tools/*.rs and rust/**/*.rs occurs in the reference's own
    sources (exactly, or as the module prefix of an observed path), or is on the explicit list rust/UNOBSERVED_PATHS.txt with its
    reason.  A path written from memory of another crate layout (round 3's `stwo_prover::core::…`) fails here."""
    R = _load_scanner()
    obs, listed = _observed(), _unobserved_listed()
    mine = R.scan([os.path.join(ROOT, "tools"), os.path.join(ROOT, "rust")])
    assert len(mine) > 60

    def observed(p):
        return p in obs or any(o.startswith(p + "::") for o in obs)
    bad = sorted(p for p in mine if not observed(p) and p not in listed and not any(l.startswith(p + "::") for l in listed))
    assert bad == [], "neither in the reference nor in rust/UNOBSERVED_PATHS.txt: %s" % bad
    stale = sorted(p for p in listed if observed(p) or not any(m == p or m.startswith(p + "::") for m in mine))
    assert stale == [], "listed as unobserved but observed in the reference, or no longer used: %s" % stale
    assert not any(p.startswith("stwo_prover") for p in mine)


def _crate_paths(R, src, parent):
    out = set()
    for m in re.finditer(r"\buse\s+([^;]+);", R.strip_comments(src), flags=re.S):
        for p in R.expand(re.sub(r"\s+", " ", m.group(1))):
            p = p.replace(" ", "")
            if p.startswith("super::"):
                p = parent + p[len("super::"):]
            if p.startswith("crate::"):
                out.add(p)
    return out


def test_reference_patch_imports_what_machine_rs_imports():
    """rust/nexus-hip/reference_patch/machine_hip.rs is a child module of the reference's `machine`: every `crate::` item it imports is one
    machine.rs itself imports (there as `super::` / `crate::`), and what it takes from its parent exists there."""
    R = _load_scanner()
    patch = open(os.path.join(HIP_DIR, "reference_patch", "machine_hip.rs")).read()
    mine = _crate_paths(R, patch, "crate::machine::")
    fixture = os.path.join(ROOT, "tests", "golden", "reference_machine_rs_use_paths.txt")
    if REFERENCE:
        ref = _crate_paths(R, _ref_src("prover/src/machine.rs"), "crate::")
        assert sorted(ref) == open(fixture).read().split(), "regenerate tests/golden/reference_machine_rs_use_paths.txt"
    ref = set(open(fixture).read().split())
    own = {p for p in mine if p.startswith("crate::machine::")}
    assert own == {"crate::machine::GeneratedTraces", "crate::machine::Machine", "crate::machine::Proof", "crate::machine::BASE_EXTENSIONS"}
    missing = sorted(p for p in mine - own if p not in ref)
    assert missing == [], missing
    if REFERENCE:
        msrc = _ref_src("prover/src/machine.rs")
        assert "const BASE_EXTENSIONS" in msrc and "pub struct Machine" in msrc and "pub struct Proof" in msrc and "fn max_log_size" in msrc


def test_prover2_patch_imports_what_prove_rs_imports():
    """rust/nexus-hip/reference_patch/prove2_hip.rs is a sibling of the reference's `prove` module in prover2/machine/src/lib.rs (SURVEY.md
    section 8(a) R2): every `crate::` / `super::` item it imports is one prove.rs itself imports, plus prove.rs's own `Proof`; the statements
    it shares with prove.rs (trace generation, channel seeding, component order) are there; what README.md edit 6 adds to
    `MachineComponent` sits next to the method it twins."""
    R = _load_scanner()
    patch = open(os.path.join(HIP_DIR, "reference_patch", "prove2_hip.rs")).read()
    mine = _crate_paths(R, patch, "crate::")
    fixture = os.path.join(ROOT, "tests", "golden", "reference_prove2_rs_use_paths.txt")
    if REFERENCE:
        ref = _crate_paths(R, _ref_src("prover2/machine/src/prove.rs"), "crate::")
        assert sorted(ref) == open(fixture).read().split(), "regenerate tests/golden/reference_prove2_rs_use_paths.txt"
    ref = set(open(fixture).read().split())
    own = {"crate::prove::Proof", "crate::prove", "crate::verify"}          # prove.rs's own items (its test module names `crate::verify` too)
    missing = sorted(p for p in mine - own if p not in ref)
    assert missing == [], missing
    assert "crate::BASE_COMPONENTS" in mine and "crate::side_note::SideNote" in mine and "crate::lookups::AllLookupElements" in mine
    for needle in ("pub fn prove_hip(trace: &impl Trace, view: &View) -> Result<Proof, ProvingError>", "c.generate_component_trace(&mut prover_side_note)",
                   "c.max_constraint_log_degree_bound(log_size) - log_size", "c.draw_lookup_elements(&mut lookup_elements, &mut host_channel)",
                   "t.to_circle_evaluation(PREPROCESSED_TRACE_IDX)", "t.to_circle_evaluation(ORIGINAL_TRACE_IDX)",
                   "interaction_tree_on_device(&mut session, &generators, [&kept0, &kept1])", "c.to_recorded_component(&mut locations, &lookup_elements, *log_size, *claimed_sum)",
                   "session.mix_felts(&claimed_words)", "session.tree_commit()", "session.prove(&recorded)", "proof_bytes(&words, &claimed_words, &log_sizes)"):
        assert needle in patch, needle
    assert "tree_commit_host(" not in patch and "generate_interaction_trace(" not in R.strip_comments(patch)   # tree 2 is generated on the device
    readme = open(os.path.join(HIP_DIR, "reference_patch", "README.md")).read()
    for needle in ("fn to_recorded_component(&self, locations: &mut nexus_hip::record::TraceLocations", "BuiltInComponentEval::<C> { component: self, log_size, lookup_elements }",
                   "mod prove_hip;", "pub use prove_hip::prove_hip;"):
        assert needle in readme, needle
    # the statements the patch shares with prove.rs
    shared = ("let mut prover_side_note = SideNote::new(trace, view);", "let components = BASE_COMPONENTS;", ".map(|c| c.generate_component_trace(&mut prover_side_note))",
              "let log_sizes: Vec<u32> = traces.iter().map(ComponentTrace::log_size).collect();", "for byte in view.view_associated_data().unwrap_or_default() {")
    for stmt in shared:
        assert stmt in patch, stmt
    if REFERENCE:
        er = _ref_src("prover2/machine/src/framework/traits/erased.rs")
        assert "pub trait MachineComponent" in er and "fn to_component_prover<'a>(" in er and "BuiltInComponentEval::<C> {" in er and "C::LookupElements::get(lookup_elements)" in er
        ev = _ref_src("prover2/machine/src/framework/eval.rs")
        assert "pub(crate) component: &'a C" in ev and "pub(crate) log_size: u32" in ev and "pub(crate) lookup_elements: C::LookupElements" in ev
        lib2 = _ref_src("prover2/machine/src/lib.rs")
        assert "const BASE_COMPONENTS: &[&dyn framework::MachineComponent]" in lib2 and "\nmod prove;" in lib2
        pr = R.strip_comments(_ref_src("prover2/machine/src/prove.rs"))
        for stmt in shared:
            assert stmt in pr, stmt


def test_the_two_reference_patches_share_their_device_steps():
    """rust/nexus-hip/src/simd_host.rs holds what machine_hip.rs and prove2_hip.rs both do with the reference's SimdBackend evaluations
    (commit while keeping the evaluations, the host channel the lookup elements are drawn from, the interaction tree from the recorded
    relation entries); neither patch carries a private copy."""
    host = open(os.path.join(HIP_DIR, "src", "simd_host.rs")).read()
    for needle in ("pub fn commit_tree_keeping_evaluations(session: &mut Session, evals: &[SimdEval], keep_mask: Option<&[bool]>)", "pub fn host_channel_at(session: &Session) -> Blake2sChannel",
                   "pub fn columns_read_by_fractions(recorded: &[RecordedComponent], n_cols: [usize; 2]) -> [Vec<bool>; 2]",
                   "pub fn interaction_tree_on_device(session: &mut Session, recorded: &[RecordedComponent], kept: [&[*const u32]; 2])", "pub fn pcs_config(config: &PcsConfig, log_constraint_degree: u32)",
                   "session.tree_commit_host(&host, false, &keep)", "session.logup_trace(c, &cols, &out)", "ch.update_digest(Blake2sHash(session.channel_digest()))"):
        assert needle in host, needle
    # only what the chips filled goes over PCIe: the provers' trees 0 and 1 (one helper), and the verifier's re-commit of tree 0 (R10)
    assert host.count("tree_commit_host(") == 2 and "pub fn preprocessed_root_on_device(config: &PcsConfig, evals: &[SimdEval]" in host
    assert "preprocessed_root_on_device(&PcsConfig::default(), &evals, max_log, LOG_CONSTRAINT_DEGREE, 0)" in open(os.path.join(HIP_DIR, "reference_patch", "README.md")).read()
    assert "#[cfg(stwo_traits)]\npub mod simd_host;" in open(HIP).read()
    for f in ("machine_hip.rs", "prove2_hip.rs"):
        patch = open(os.path.join(HIP_DIR, "reference_patch", f)).read()
        assert "use nexus_hip::simd_host::{columns_read_by_fractions, commit_tree_keeping_evaluations, host_channel_at, interaction_tree_on_device, pcs_config, secure_from_words, SimdEval};" in patch, f
        # only the columns the fraction programs read stay on the device beyond their commit, and they go before the prove
        assert "AllLookupElements::dummy()" in patch and "Some(&reads[0])" in patch and "Some(&reads[1])" in patch and "session.free_columns();" in patch, f
        for private in ("fn commit_tree_keeping_evaluations", "fn interaction_tree_on_device", "fn host_channel_at", "sys::nx_pcs_config {"):
            assert private not in patch, (f, private)


BACKEND_TRAITS = ["Backend", "BackendForChannel<Blake2sMerkleChannel>", "ColumnOps<BaseField>", "ColumnOps<SecureField>", "ColumnOps<Blake2sHash>",
                  "FieldOps<BaseField>", "FieldOps<SecureField>", "PolyOps", "MerkleOps<Blake2sMerkleHasher>", "QuotientOps", "FriOps", "AccumulationOps",
                  "GrindOps<Blake2sChannel>", "GkrOps", "MleOps<BaseField>", "MleOps<SecureField>"]
TRAIT_METHODS = {   # the methods a backend must provide, and the crate::ops adapter each rests on
    "PolyOps": {"new_canonical_ordered": "finalize_columns", "interpolate": "interpolate", "interpolate_columns": "interpolate", "eval_at_point": "eval_at_points",
                "extend": "nx_copy", "evaluate": "evaluate", "evaluate_polynomials": "evaluate", "precompute_twiddles": "precompute_twiddles"},
    "MerkleOps<Blake2sMerkleHasher>": {"commit_on_layer": "commit_on_layer"},
    "QuotientOps": {"accumulate_quotients": "accumulate_quotients"},
    "FriOps": {"fold_line": "fold_line", "fold_circle_into_line": "fold_circle_into_line", "decompose": "fri_decompose"},
    "AccumulationOps": {"accumulate": "secure_accumulate", "generate_secure_powers": "generate_secure_powers"},
    "GrindOps<Blake2sChannel>": {"grind": "grind"},
    "FieldOps<BaseField>": {"batch_inverse": "batch_inverse_m31"},
    "FieldOps<SecureField>": {"batch_inverse": "batch_inverse_qm31"},
    "ColumnOps<BaseField>": {"bit_reverse_column": "bit_reverse"},
    "ColumnOps<SecureField>": {"bit_reverse_column": "bit_reverse_secure"},
}


def _impl_body(src, header):
    i = src.index(header)
    j = src.index("{", i)
    depth, k = 1, j + 1
    while depth:
        depth += src[k] == "{"
        depth -= src[k] == "}"
        k += 1
    return src[j + 1:k - 1]


def test_every_backend_trait_has_its_impl_for_hipbackend():
    """the trait impls stopped after ColumnOps.  Every trait stwo::prover::prove is generic over (Backend's supertraits and
    BackendForChannel's bounds) has an `impl … for HipBackend` in rust/nexus-hip/src/backend.rs, every required method is there and goes
    through the `ops::` adapter (hence the C-ABI export) INTEGRATION.md names for it; the recorded component implements ComponentProver."""
    src = open(os.path.join(HIP_DIR, "src", "backend.rs")).read()
    ops_src = open(HIP).read()
    ops_fns = set(re.findall(r"pub fn (\w+)\(", _impl_body(ops_src, "pub mod ops")))
    for t in BACKEND_TRAITS:
        assert ("impl %s for HipBackend" % t) in src, t
    for t, methods in TRAIT_METHODS.items():
        body = _impl_body(src, "impl %s for HipBackend" % t)
        for m, adapter in methods.items():
            mm = re.search(r"fn %s\b" % m, body)
            assert mm, (t, m)
            nxt = re.search(r"\n    fn \w+", body[mm.end():])
            mbody = body[mm.end():mm.end() + nxt.start()] if nxt else body[mm.end():]
            if adapter.startswith("nx_"):
                assert "sys::" + adapter in mbody, (t, m, adapter)
            else:
                assert adapter in ops_fns and ("ops::" + adapter) in mbody, (t, m, adapter)
    for col_t in ("BaseField", "SecureField", "Blake2sHash"):
        body = _impl_body(src, "impl Column<%s> for HipColumn<%s>" % (col_t, col_t))
        for m in ("zeros", "uninitialized", "to_cpu", "len", "at", "set"):
            assert re.search(r"fn %s\b" % m, body), (col_t, m)
        assert ("impl FromIterator<%s> for HipColumn<%s>" % (col_t, col_t)) in src
    assert "impl<C: stwo::core::air::Component> ComponentProver<HipBackend> for HipComponent<C>" in src
    assert "ops::air_eval(" in _impl_body(src, "impl<C: stwo::core::air::Component> ComponentProver<HipBackend> for HipComponent<C>")
    # no trait is left as a comment any more
    assert "one adapter each over" not in ops_src and "unimplemented!" not in _impl_body(src, "impl PolyOps for HipBackend")


def test_recording_evaluator_lowers_to_the_abi_opcodes():
    """rust/nexus-hip/src/record.rs: the recording EvalAtRow exists as code — associated types, the trait methods the reference's AIR
    calls (trace/eval.rs:22-50, components/mod.rs:48-56), the lowering to every NX_C_* opcode of include/nexus_hip.h, the linear-scan
    allocation — and mirrors air_program.py's rules (chunks of 8 constraints, canonical operand order of commutative ops)."""
    src = open(os.path.join(HIP_DIR, "src", "record.rs")).read()
    for needle in ("impl<'a> EvalAtRow for RecordingEval<'a>", "type F = F;", "type EF = EF;", "fn next_interaction_mask<const N: usize>", "fn get_preprocessed_column",
                   "fn add_constraint<G>", "fn combine_ef", "logup_proxy!()", "pub fn record_component<E: FrameworkEval>", "const CHUNK: usize = 8;", "a.min(c), a.max(c)"):
        assert needle in src, needle
    header_ops = re.findall(r"#define (NX_C_\w+)", open(HEADER).read()) or re.findall(r"\b(NX_C_[A-Z_]+)\b\s*=", open(HEADER).read())
    assert len(set(header_ops)) == 17            # 15 constraint-program opcodes + NX_C_FRAC / NX_C_FRACB (the relation entries' fraction program)
    for op in set(header_ops):
        assert "sys::" + op in src, op
    patch = open(os.path.join(HIP_DIR, "reference_patch", "machine_hip.rs")).read()
    for needle in ("pub fn prove_hip(trace: &impl Trace, view: &View) -> Result<Proof, ProvingError>", "record_component(", "session.prove(&components)", "proof_bytes(",
                   "generate_interaction_trace::<C>(", "C::draw_lookup_elements(",
                   # the interaction tree is generated on the device from the recorded relation entries; tree 2 is never uploaded
                   "interaction_tree_on_device(&mut session, &generators, [&kept0, &kept1])", "session.tree_commit()"):
        assert needle in patch, needle
    assert patch.count("commit_tree_keeping_evaluations(&mut session, &tree") == 2 and "&tree2" not in patch      # only trees 0 and 1 go over PCIe
    for needle in ("fn add_to_relation<R: Relation<F, EF>>", "self.rec.fracs.push(", "Root::Frac {", "sys::NX_C_FRAC", "sys::NX_C_FRACB", "logup_program, logup_n_regs"):
        assert needle in src, needle
    lib = open(os.path.join(HIP_DIR, "src", "lib.rs")).read()
    for needle in ("pub fn logup_trace(&mut self, comp: &RecordedComponent", "sys::nx_logup_program(", "sys::nx_logup_finalize_last(", "pub fn alloc_columns(", "sys::nx_comm_group_reset("):
        assert needle in lib, needle


def test_rust_sources_are_lexically_balanced():
    """No compiler here: at least every bracket closes (outside strings, chars and comments) in every Rust file we ship."""
    files = dict(_hand_written_sources())
    files["tools/dump_reference.rs"] = open(os.path.join(ROOT, "tools", "dump_reference.rs")).read()
    files["rust/nexus-hip-sys/src/lib.rs"] = open(SYS).read()
    assert len(files) >= 6
    for name, src in files.items():
        t = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        t = re.sub(r"//[^\n]*", "", t)
        t = re.sub(r'"(?:\\.|[^"\\])*"', '""', t)
        t = re.sub(r"'(?:\\.|[^'\\])'", "' '", t)          # char literals (lifetimes have no closing quote and stay)
        stack = []
        pairs = {")": "(", "]": "[", "}": "{"}
        for ch in t:
            if ch in "([{":
                stack.append(ch)
            elif ch in ")]}":
                assert stack and stack[-1] == pairs[ch], (name, ch)
                stack.pop()
        assert not stack, (name, stack[-3:])
