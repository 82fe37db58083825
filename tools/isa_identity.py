#!/usr/bin/env python3
"""Are two device assembly files (hipcc -save-temps, *-hip-amdgcn-amd-amdhsa-gfx950.s) the same code, function by function?
Functions are keyed by mangled name; what depends only on the order of definition is normalised away: the function index in
.LBB<i>_<j> / .LJTI<i>_<j> / .Lfunc_begin<i> / .Lfunc_end<i> labels, .loc / .file / .cfi and comment lines, trailing comments, and
the order of the functions in the file.  What is compared is the instruction stream and, for kernels, the whole .amdhsa_kernel
block (registers, LDS, scratch).  argv: before.s after.s [-v] [--rename REGEX REPL]; exit status 1 if anything differs or is
missing.  --rename rewrites the text of after.s first (re.sub): a kernel template that gained a parameter has new mangled names, and
its old instances are compared under their old ones."""
import difflib, re, sys

RENAME = (sys.argv[sys.argv.index('--rename') + 1], sys.argv[sys.argv.index('--rename') + 2]) if '--rename' in sys.argv else None

def functions(path, rename=None):
    s = open(path).read()
    if rename:
        s = re.sub(rename[0], rename[1], s)
    out = {}
    for m in re.finditer(r'^(\S+):[ \t]*; @\1\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M):
        body = []
        for ln in m.group(2).split('\n'):
            t = ln.split(';')[0].rstrip()
            if not t.strip() or re.match(r'\s*\.(loc|file|cfi_\w+)\b', t):
                continue
            body.append(re.sub(r'\.(LBB|LJTI|Lfunc_begin|Lfunc_end|Ltmp)\d+', r'.\1', t))
        out[m.group(1)] = (body, '.amdhsa_kernel ' + m.group(1) in m.group(2))
    return out

a, b = functions(sys.argv[1]), functions(sys.argv[2], RENAME)
missing = sorted(set(a) - set(b))
added = sorted(set(b) - set(a))
differ = sorted(n for n in a if n in b and a[n][0] != b[n][0])
kernels = sum(1 for n in a if a[n][1])
print('%d kernels, %d other functions before; %d missing after, %d new after, %d differ'
      % (kernels, len(a) - kernels, len(missing), len(added), len(differ)))
for tag, names in (('missing', missing), ('new', added), ('differs', differ)):
    for n in names:
        print('  %s: %s' % (tag, n))
        if tag == 'differs' and '-v' in sys.argv:
            sys.stdout.write('\n'.join(list(difflib.unified_diff(a[n][0], b[n][0], 'before', 'after', lineterm='', n=1))[:60]) + '\n')
sys.exit(1 if missing or differ else 0)
