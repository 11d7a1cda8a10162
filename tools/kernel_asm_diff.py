"""Which kernels of a translation unit kept their instructions across a change:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S FILE.hip -o BEFORE.s     (on the parent)
    hipcc ... -S FILE.hip -o AFTER.s                                                           (on this tree)
    python tools/kernel_asm_diff.py BEFORE.s AFTER.s
Per kernel: comments and directives stripped, basic-block labels renumbered, names demangled."""
import re, sys, hashlib
import subprocess
def key(mangled):
    # demangled name and template arguments; the rank-2 flag this tree adds as a last, defaulted argument is dropped where
    # it is false, so that an existing instance keeps its parent's name
    d = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    d = d.replace('void ', '').replace('sgpr::(anonymous namespace)::', '')
    d = re.sub(r'\(.*$', '', d)
    m = re.match(r'(nllgrad_(?:pairs|reg)_kernel)<(.*)>$', d)
    if m:
        args = m.group(2).split(', ')
        want = 3 if 'pairs' in m.group(1) else 2
        if len(args) == want + 1:
            d = '%s<%s>' % (m.group(1), ', '.join(args[:want])) + (' rank-2' if args[-1] == 'true' else '')
    return d
def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m and 'kernel' in m.group(1):
            name = key(m.group(1)); cur = []; out[name] = cur; continue
        if cur is not None:
            if line.startswith('.Lfunc_end'):
                cur = None; continue
            t = line.split(';')[0].rstrip()
            if not t.strip() or t.strip().startswith('.'):
                if not re.match(r'^\.LBB', t.strip()): continue
            t = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', t)
            cur.append(t)
    return out
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
print("kernels: parent %d, this tree %d" % (len(a), len(b)))
bad = 0
for k in sorted(a):
    if k not in b: print("MISSING", k); bad += 1; continue
    same = a[k] == b[k]
    bad += not same
    print("%s  %5d instr+labels  sha1 %s  %s" % ("same" if same else "DIFF", len(a[k]), hashlib.sha1("\n".join(b[k]).encode()).hexdigest()[:12], k))
for k in sorted(set(b) - set(a)): print("new   %5d instr+labels  %s" % (len(b[k]), k))
print("existing instances that differ: %d" % bad)
