"""The compiler's kernel-resource-usage remarks of one source file (csrc/build/X_resources.txt, written by the build), as the
tests/test_*_resources.py files read them."""
import re


def _kernels(path):
    """mangled kernel name -> {remark label: integer value}"""
    out, cur = {}, None
    for line in path.read_text().splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out
