"""Are the kernels of two ISA listings the same, kernel by kernel?

    python tools/debug/isa_kernel_equal.py OLD.s NEW.s [--gone SUBSTRING ...]

For every kernel symbol of two listings (hipcc -S --cuda-device-only) compares the whole text of its body -- comments dropped,
local labels `.LBB<function index>_` renumbered, since the index shifts when a kernel in front appears or disappears -- and its
`.amdhsa_*` descriptor block (LDS, registers, scratch, ...).  Prints one verdict line per symbol and fails unless every common
kernel is the same and the symbols found in one listing only are exactly the OLD ones that match a `--gone` substring.
A refactor that must not change device code is checked with this (isa_block_diff.py is for changes that may)."""
import argparse
import re
import sys


def kernels(path):
    """symbol -> (body lines, descriptor lines)"""
    lines = open(path).read().split('\n')
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == '.end_amdhsa_kernel')
        desc = [' '.join(l.split()) for l in lines[i + 1:end]]
        start = max(j for j in range(i) if lines[j].startswith(sym + ':'))
        body = []
        for l in lines[start + 1:i]:
            t = re.sub(r'\.LBB\d+_', '.LBB_', ' '.join(l.split(';')[0].split()))
            if t:
                body.append(t)
        out[sym] = (body, desc)
    return out


def ninstr(body):
    return sum(not (t.startswith('.') or t.endswith(':')) for t in body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--gone', action='append', default=[], help='substring of a kernel symbol that must be in OLD only')
    a = ap.parse_args()
    ko, kn = kernels(a.old), kernels(a.new)
    bad = 0
    for sym in ko:
        if sym not in kn:
            ok = any(g in sym for g in a.gone)
            bad += not ok
            print(f'{sym}  {ninstr(ko[sym][0])} instructions  {"gone, as intended" if ok else "MISSING in new"}')
            continue
        same_body, same_desc = ko[sym][0] == kn[sym][0], ko[sym][1] == kn[sym][1]
        bad += not (same_body and same_desc)
        print(f'{sym}  {ninstr(ko[sym][0])} instructions  ' + ('same' if same_body and same_desc else
              f'DIFFERENT ({"body" if not same_body else ""}{" descriptor" if not same_desc else ""}; new has {ninstr(kn[sym][0])} instructions)'))
    for sym in kn:
        if sym not in ko:
            bad += 1
            print(f'{sym}  {ninstr(kn[sym][0])} instructions  NEW-ONLY')
    common = sum(s in kn for s in ko)
    print(f'# {common} kernels in both listings, {common - sum(ko[s] != kn[s] for s in ko if s in kn)} the same; '
          f'{sum(s not in kn for s in ko)} in old only, {sum(s not in ko for s in kn)} in new only')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
