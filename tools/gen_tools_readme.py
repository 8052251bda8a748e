#!/usr/bin/env python
"""Regenerate tools/README.md: one row per script in tools/ (and tools/probe/)
from its module docstring (Python) or its leading comment block (shell, HIP).

    python tools/gen_tools_readme.py
"""
import ast
import os

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD = """# tools/ — benchmarks, probes and profiling scripts

Benchmarks and probes behind the files under `profiles/`. `prof_*.sh` are `gpurun` command scripts; the one-shot
checkpoint scripts of rounds 1-5 are archived in `profiles/scripts/`; `run_steps.sh` chains GPU steps with
per-step time limits and stops at the first fault. The Python tools run on one GPU unless noted. Generated from each
file's docstring or header comment by `tools/gen_tools_readme.py`.

| File | What it does |
|---|---|
"""

TAIL = """
## Input forms on the host -> HBM link

`pack_bytes.py` and `copy_timeline.py` report on the forms a pinned `SplitStore` keeps for re-staging (raw, k-bit
codes, dictionary codes). The formats, the knobs (`MR_PACK_INPUT`, `MR_PACK_DICT`) and what each form costs are in
`docs/GUIDE.md` (the `MR_PACK_INPUT` and `MR_PACK_DICT` entries); the measurements are in
`profiles/input_pack/README.md` and `profiles/input_dict/README.md`. `bench_invidx.py` and the bigram job of
`bench_generic.py` are not bound by the link and ship k-bit codes unless run with `--pack-dict`.
"""


def describe(path: str) -> str:
    text = open(path, encoding="utf-8", errors="replace").read()
    if path.endswith(".py"):
        try:
            doc = ast.get_docstring(ast.parse(text)) or ""
        except SyntaxError:
            doc = ""
    else:
        lines = []
        for ln in text.splitlines():
            s = ln.strip()
            if s.startswith("#!"):
                continue
            if s.startswith("#") or s.startswith("//"):
                lines.append(s.lstrip("#/ ").strip())
            elif lines or s:
                break
        doc = " ".join(x for x in lines if x)
    doc = " ".join(doc.split())
    return (doc[:217] + " ...") if len(doc) > 220 else (doc or "(no description)")


def main() -> None:
    rows = []
    for sub in ("", "probe"):
        d = os.path.join(HERE, sub)
        for name in sorted(os.listdir(d)):
            p = os.path.join(d, name)
            if os.path.isfile(p) and name.endswith((".py", ".sh", ".hip")) and name != "README.md":
                rows.append(f"| `{os.path.join(sub, name) if sub else name}` | {describe(p).replace('|', '/')} |")
    with open(os.path.join(HERE, "README.md"), "w") as f:
        f.write(HEAD + "\n".join(rows) + "\n" + TAIL)


if __name__ == "__main__":
    main()
