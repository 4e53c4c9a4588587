"""What the test_kernel_table_*.py files share: tools/kernel_table.py as a module, and a kernel's instruction lines from the compiler's
own listing (hipcc -S for gfx950 with the library's flags, no GPU needed) with the small parsers the files read it by."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "zeldaengine_amd", "csrc", "zr_lighting.hip")


def kernel_table():
    spec = importlib.util.spec_from_file_location("kernel_table", os.path.join(ROOT, "tools", "kernel_table.py"))
    kt = importlib.util.module_from_spec(spec); spec.loader.exec_module(kt)
    return kt


def listing(tmp, kernel, extra=()):
    """the lines (comments kept) of the one kernel of csrc/zr_lighting.hip whose demangled name starts with `kernel`, built with `extra` flags"""
    kt = kernel_table()
    out = os.path.join(str(tmp), "l%d.s" % len(extra))
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip"] + kt.FLAGS + list(extra) + ["-o", out, SRC], stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    name = [n for n, d in zip(names, plain) if d.replace("void ", "").startswith(kernel)]
    assert len(name) == 1, plain
    body = text[text.index("\n" + name[0] + ":"):]
    return body[:body.index(".Lfunc_end")].split("\n")


def ops(lines):
    """[(line number, the line's words)] of the instructions: comments, directives and blank lines left out"""
    return [(n, l.split()) for n, l in enumerate(lines) if l.strip() and l.strip()[0] not in ";."]


def labels(lines):
    """{label of a basic block: its line number}"""
    return {l.split(":")[0]: n for n, l in enumerate(lines) if re.match(r"\.LBB\S+:", l)}
