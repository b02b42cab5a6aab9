"""Per-symbol comparison of two gfx950 device assemblies of one source file (e.g. csrc/pairwise.hip before and after a change).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S old/pairwise.hip -o old.s     (the Makefile's flags)
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S new/pairwise.hip -o new.s
    python tools/isa_diff.py old.s new.s [--json out.json]

For every function symbol the instruction stream is taken (labels and instructions; directives, comments and blank lines
dropped) and hashed.  Prints how many symbols of OLD are in NEW with the same instructions, lists every one that differs
or is gone, and the symbols only NEW has with their instruction counts.  Exit status 1 if an OLD symbol differs or is gone.
"""
import argparse
import hashlib
import json
import re
import sys

_FUNC = re.compile(r'^\s*\.type\s+([\w$.]+),@function')
_LABEL = re.compile(r'\.LBB\d+_(\d+)')


def functions(path):
    """{symbol: [instruction or label lines]} of an assembly file."""
    lines = open(path).read().splitlines()
    names = {m.group(1) for m in map(_FUNC.match, lines) if m}
    out, cur = {}, None
    for ln in lines:
        # .LBB<function number>_<block>: the function number is its position in the file, not part of the code
        body = _LABEL.sub(r'.LBB_\1', ln.split(';', 1)[0].rstrip())
        if not body.strip():
            continue
        if not body[0].isspace() and body.endswith(':'):
            lab = body[:-1]
            if lab in names:
                cur = out.setdefault(lab, [])
                continue
            if lab.startswith('.Lfunc_end'):
                cur = None
                continue
            if cur is not None:
                cur.append(body)
            continue
        if cur is None or body.strip().startswith('.'):
            continue
        cur.append(' '.join(body.split()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--json')
    a = ap.parse_args()
    old, new = functions(a.old), functions(a.new)
    h = lambda body: hashlib.sha256('\n'.join(body).encode()).hexdigest()[:16]  # noqa: E731
    same = [s for s in old if s in new and old[s] == new[s]]
    changed = [s for s in old if s in new and old[s] != new[s]]
    gone = [s for s in old if s not in new]
    added = {s: sum(1 for ln in new[s] if not ln.endswith(':')) for s in new if s not in old}
    print(f'old: {len(old)} symbols, new: {len(new)} symbols')
    print(f'identical instruction streams: {len(same)} of {len(old)}')
    for s in changed:
        print(f'CHANGED {s}: {h(old[s])} -> {h(new[s])}')
    for s in gone:
        print(f'GONE    {s}')
    print(f'only in new: {len(added)}')
    for s, n in sorted(added.items()):
        print(f'  {n:6d} instructions  {s}')
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'old_symbols': len(old), 'new_symbols': len(new), 'identical': len(same), 'changed': changed,
                       'gone': gone, 'added': added, 'hashes': {s: h(new[s]) for s in sorted(new)}}, f, indent=1)
    return 1 if changed or gone else 0


if __name__ == '__main__':
    sys.exit(main())
