"""Every context option of the table in csrc/ctx.hip is (a) named in the option paragraph of include/nexus_hip.h, whose last sentence
promises that no option changes a result, and (b) actually set by some GPU test, so that the promise is held to on the device."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def option_table():
    """{option name: NX_* variable that seeds it (None: no variable)} from k_options / options_from_env of csrc/ctx.hip."""
    src = _read("nexus-zkvm_amd", "csrc", "ctx.hip")
    table = src[src.index("static const OptEntry k_options[]"):]
    table = table[:table.index("};")]
    fields = dict(re.findall(r'\{"([a-z0-9_.]+)",\s*&nx_options::(\w+),', table))
    env = dict(re.findall(r'\bo\.(\w+)\s*=[^;]*?env_int\("(NX_[A-Z0-9_]+)"', src))
    return {name: env.get(field) for name, field in fields.items()}


def test_the_option_table_is_found():
    opts = option_table()
    assert len(opts) >= 24 and {"fft.kmax", "merkle.pair_levels", "machine.reuse_preprocessed", "host.pack_threads"} <= set(opts)
    assert opts["fft.kmax"] == "NX_FFT_KMAX" and opts["host.pack_threads"] is None


def test_every_option_is_named_in_the_headers_option_paragraph():
    hdr = _read("include", "nexus_hip.h")
    end = hdr.index("int nx_ctx_set_option(")
    para = hdr[hdr.rindex("/*", 0, end):end]
    assert "bit-identical under every setting" in para
    missing = [name for name in option_table() if f'"{name}"' not in para]
    assert not missing, f"options of csrc/ctx.hip the header's option paragraph does not name: {missing}"


def _options_set_by(path):
    """Option names a test file sets: string literals given to set_option, the keys of dict literals in a file that also calls set_option
    with a computed name (settings tables applied in a loop), and NX_* variables given to setenv."""
    tree = ast.parse(_read(path))
    names, variables, computed = set(), set(), False
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.args:
            first = node.args[0]
            literal = first.value if isinstance(first, ast.Constant) and isinstance(first.value, str) else None
            if node.func.attr == "set_option":
                if literal is None:
                    computed = True
                else:
                    names.add(literal)
            elif node.func.attr == "setenv" and literal:
                variables.add(literal)
    if computed:
        for node in ast.walk(tree):
            if isinstance(node, ast.Dict):
                names |= {k.value for k in node.keys if isinstance(k, ast.Constant) and isinstance(k.value, str)}
    return names, variables


def test_every_option_is_set_by_some_gpu_test():
    names, variables = set(), set()
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert files
    for f in files:
        n, v = _options_set_by(os.path.relpath(f, ROOT))
        names |= n; variables |= v
    unset = [name for name, var in option_table().items() if name not in names and var not in variables]
    assert not unset, f"options no tests/test_gpu_*.py sets (set_option or its NX_* variable): {unset}"
