"""tests/oom_sites.py against the sources: every place that takes a block from the context's caching allocator has its row (who gives the
earlier blocks back when this request is refused, what the caller sees), the budget and injection options are in the allocator and in
the header's option paragraph with the rule after NX_ERR_OOM, and a NULL context refuses them without a device."""
import collections
import ctypes as C
import os
import re

import oom_sites as S
import poison_sites as PS

NX_ERR_ARG = -2
NEW_OPTIONS = ("mem.limit_bytes", "mem.cache_bytes", "mem.cached_bytes", "debug.fail_alloc", "debug.alloc_count")


def _read(*parts):
    with open(os.path.join(S.ROOT, *parts)) as f:
        return f.read()


def test_the_scanner_is_the_poison_audits():
    assert S.scan_sites is PS.scan_sites and S.CSRC == PS.CSRC


def test_every_allocation_site_has_its_row():
    sites = S.scan_sites()
    rows = collections.Counter()
    for s in S.TABLE:
        rows[(s.file, s.function)] += s.calls
    assert len(rows) == len(S.TABLE), "two rows for one function"
    without = {k: v for k, v in sites.items() if k not in rows}
    assert not without, f"allocation sites without a row in tests/oom_sites.py (say who frees the earlier blocks when this one is refused): {without}"
    stale = {k: v for k, v in rows.items() if k not in sites}
    assert not stale, f"rows of tests/oom_sites.py whose function takes no block any more: {stale}"
    differ = {k: (sites[k], rows[k]) for k in sites if sites[k] != rows[k]}
    assert not differ, f"(calls in the sources, calls in the row): {differ}"


def test_the_two_audits_list_the_same_sites():
    assert {(s.file, s.function): s.calls for s in S.TABLE} == {(s.file, s.function): s.calls for s in PS.TABLE}


def test_every_row_names_an_owner_and_what_the_caller_sees():
    for s in S.TABLE:
        for text in (s.owner, s.caller_sees):
            assert isinstance(text, str) and len(text.strip()) > 8, s
            assert not re.search(r":\d+", text), f"{s.function}: rows cite names, not lines"
        assert s.tolerates is None or (isinstance(s.tolerates, str) and s.tolerates.strip()), s
    # a function that takes more than one block has somebody to give the earlier ones back
    for s in S.TABLE:
        if s.calls > 1:
            assert not s.owner.startswith("none earlier"), s


def test_tolerating_sites_and_entries_go_together():
    hdr = _read("include", "nexus_hip.h")
    assert bool(S.TOLERATING_ENTRIES) == any(s.tolerates for s in S.TABLE)
    for name, why in S.TOLERATING_ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % re.escape(name), hdr) and why.strip(), name


def test_the_names_the_rows_cite_exist():
    src = "".join(_read("nexus-zkvm_amd", "csrc", f) for f in sorted(os.listdir(S.CSRC)) if f.endswith((".hip", ".h", ".cuh")))
    missing = []
    for s in S.TABLE:
        for text in (s.owner, s.caller_sees):
            for name in re.findall(r"\b(?:nx_\w+|dev_free|DevBuf|SecureColumn|RootPipe|HostFeed::\w+|TreeBuilder(?:::\w+)?|PipeGuard|TwGuard|EvalJob|eval_at_points_collect|FriLayer|FriProver|"
                                   r"TreeRef|EvalDomainCols|CommitmentTreeProver|CommitmentSchemeProver|abort_peers|HalfGroup|upload_columns|prove_core|prove_synth|twiddle_kernel)\b", text):
                if not re.search(r"\b%s\b" % re.escape(name.split("::")[-1]), src):
                    missing.append((s.function, name))
    assert not missing, f"cited, but nowhere under csrc/: {missing}"


def test_the_options_are_in_the_allocator_and_in_the_header():
    ctx_src, src, hdr, internal = (_read("nexus-zkvm_amd", "csrc", "ctx.hip"), _read("nexus-zkvm_amd", "csrc", "mem.hip"), _read("include", "nexus_hip.h"),
                                   _read("nexus-zkvm_amd", "csrc", "internal.h"))
    end = hdr.index("int nx_ctx_set_option(")
    para = hdr[hdr.rindex("/*", 0, end):end]
    for name in NEW_OPTIONS:
        assert f'"{name}"' in src and f'"{name}"' in para, name
    assert "AFTER NX_ERR_OOM" in para and "NX_MEM_LIMIT_BYTES" in para and 'env_bytes("NX_MEM_LIMIT_BYTES", 0)' in src
    assert "(size_t)192 << 30" in internal and "(size_t)192 << 30" not in ctx_src + src, "the cache cap is the option's default, not a constant of dev_free"
    alloc = ctx_src[ctx_src.index("int dev_alloc(nx_ctx* ctx"):ctx_src.index("void dev_free(nx_ctx* ctx")]
    assert alloc.index("dev_alloc_admit(") < alloc.index("free_blocks.find(") < alloc.index("dev_alloc_make_room(") < alloc.index("hipMalloc("), "refusals are decided before the cache and the driver are asked"
    assert "hipMalloc" not in src and "hipLaunch" not in src, "mem.hip decides on the host"
    assert "mem_option_set(ctx, name, value, &rc)" in ctx_src and "mem_option_get(ctx, name, value)" in ctx_src and "mem_options_from_env(&o)" in ctx_src
    rule = _read("nexus-zkvm_amd", "csrc", "machine.hip")
    rule = rule[rule.index("static void abort_peers("):]
    assert "(ctx->comm_entered || rc != NX_ERR_ARG)" in rule[:rule.index("\n}")]
    assert "no peer can be waiting" not in internal


def test_a_null_context_refuses_the_new_options():
    import nexus_zkvm_amd as nz
    L = nz.load_library()
    v = C.c_int64(7)
    for name in NEW_OPTIONS:
        assert L.nx_ctx_set_option(None, name.encode(), C.c_int64(1)) == NX_ERR_ARG, name
        assert b"NULL argument" in L.nx_last_error(None)
        assert L.nx_ctx_get_option(None, name.encode(), C.byref(v)) == NX_ERR_ARG and v.value == 7, name
