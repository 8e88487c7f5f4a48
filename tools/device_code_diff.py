#!/usr/bin/env python3
"""Are two device-assembly files of the library the same code?  For a change that must not touch the device code (a move of
source between the sections csrc/ims_*.h, a host-side refactor): compile both trees with

   hipcc <flags of __graft_entry__ without -fPIC -shared> --cuda-device-only -S imsim_amd/csrc/imsim_hip.hip -o X.s

and run  python tools/device_code_diff.py A.s B.s  (exit code 1 on any difference).

The order in which the compiler emits functions, and with it the ordinals in its local labels, follows the order of the source;
the code does not.  So the files are split by symbol (`.type NAME,@function` / `@object` up to `.size NAME` and the `.set NAME.*`
lines behind it), the function ordinal is taken out of `.LBB<n>_<m>`, `.LJTI<n>_<m>`, `.LCPI<n>_<m>`, `.Lfunc_end<n>`, `.Ltmp<n>`
is numbered from zero inside each symbol, and comments and blank lines are dropped.  Compared are: the set of symbols, the text
of each symbol, the lines between symbols as a multiset, and the per-kernel records of the `amdhsa.kernels` metadata as a set
keyed by `.name`.  The `__hip_cuid_<hash>` symbol is a hash of the compilation and is compared by its prefix only."""
import collections
import re
import sys


def _clean(line):
    if '"' not in line:
        line = line.split(";")[0]
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_*", line.rstrip())
    line = re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def parse(path):
    """-> (symbols: name -> [lines], glue: Counter of the lines outside symbols, kernels: .name -> [lines], rest of the metadata)"""
    text = open(path).read().splitlines()
    meta_at = next((k for k, l in enumerate(text) if l.strip() == ".amdgpu_metadata"), len(text))
    symbols, glue = {}, collections.Counter()
    name, body, tmp, closing, own_set, own_size = None, None, {}, False, None, None
    for raw in text[:meta_at]:
        line = _clean(raw)
        if not line.strip():
            continue
        m = re.match(r"\s*\.type\s+([^,\s]+),@(function|object)", line)
        if m or (closing and not own_set.match(line)):
            name, closing = None, False
        if m:
            name, body, tmp = m.group(1), [], {}
            symbols[name] = body
            own_set = re.compile(r"\s*\.set\s+" + re.escape(name) + r"\.")
            own_size = re.compile(r"\s*\.size\s+" + re.escape(name) + r"\s*,")
        if name is None:
            glue[line.strip()] += 1
            continue
        body.append(re.sub(r"\.Ltmp(\d+)", lambda t: ".Ltmp%d" % tmp.setdefault(t.group(1), len(tmp)), line))
        if own_size.match(line):
            closing = True
    kernels, rest, rec = {}, [], None
    for raw in text[meta_at:]:
        if raw.startswith("  - "):
            rec = []
            rest.append(rec)
        elif not raw.startswith(" "):
            rec = None
        (rest if rec is None else rec).append(raw.rstrip())
    other = []                                  # the metadata outside the kernel records, in order
    for rec in rest:
        key = next((l.split(":", 1)[1].strip() for l in rec if l.strip().startswith(".name:")), None) if isinstance(rec, list) else None
        if key is not None:
            kernels[key] = rec
        else:
            other += rec if isinstance(rec, list) else [rec]
    return symbols, glue, kernels, other


def _first_difference(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"line {k + 1} of the symbol: {x.strip()!r} -> {y.strip()!r}"
    return f"{len(a)} -> {len(b)} lines"


def compare(path_a, path_b):
    """-> list of (kind, name, detail); kinds: only_in_a, only_in_b, text, between, kernel_only_in_a, kernel_only_in_b,
    kernel_record, metadata.  Empty: the same device code."""
    sa, ga, ka, ra = parse(path_a)
    sb, gb, kb, rb = parse(path_b)
    out = [("only_in_a", n, "") for n in sa if n not in sb] + [("only_in_b", n, "") for n in sb if n not in sa]
    out += [("text", n, _first_difference(sa[n], sb[n])) for n in sa if n in sb and sa[n] != sb[n]]
    out += [("between", l, f"{ga[l]} -> {gb[l]} times") for l in sorted(set(ga) | set(gb)) if ga[l] != gb[l]]
    out += [("kernel_only_in_a", n, "") for n in ka if n not in kb] + [("kernel_only_in_b", n, "") for n in kb if n not in ka]
    for n in ka:
        if n in kb and ka[n] != kb[n]:
            changed = [f"{x.strip()} -> {y.strip()}" for x, y in zip(ka[n], kb[n]) if x != y] or [f"{len(ka[n])} -> {len(kb[n])} lines"]
            out.append(("kernel_record", n, "; ".join(changed[:4])))
    if ra != rb:
        out.append(("metadata", "", _first_difference(ra, rb)))
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    diffs = compare(sys.argv[1], sys.argv[2])
    symbols, _, kernels, _ = parse(sys.argv[1])
    print(f"{len(symbols)} symbols and {len(kernels)} kernel records in {sys.argv[1]}: "
          + ("no difference" if not diffs else f"{len(diffs)} differences") + " (__hip_cuid_* compared by its prefix)")
    for kind, name, detail in diffs[:50]:
        print(f"  {kind}: {name} {detail}")
    sys.exit(1 if diffs else 0)
