#!/usr/bin/env python3
"""Per-kernel assembly of two builds of one source, compared kernel by kernel (instructions and .amdhsa metadata; comments,
label numbers and symbol names normalised).  A kernel that gained a trailing `float` template argument (the storage type of the
bf16 edge change) is matched to its old name.  Prints the kernels that differ and a count line.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -c egt_amd/csrc/egt_ffn.hip -I egt_amd/csrc -I include \
          -mllvm -amdgpu-mfma-vgpr-form=1 --save-temps=obj -o /tmp/new/egt_ffn.o        (and the same for the parent commit's tree)
    python tools/cmp_kernel_asm.py /tmp/old/egt_ffn-hip-amdgcn-amd-amdhsa-gfx950.s /tmp/new/egt_ffn-hip-amdgcn-amd-amdhsa-gfx950.s [-v]
"""
import re, subprocess, sys

def funcs(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\S+):\s*(;.*)?$', line)
        if m and not line.startswith('.'):
            name = m.group(1); cur = []; out[name] = cur; continue
        if name is None: continue
        if re.match(r'^\s*\.(end_amdhsa_kernel|size)\b', line):
            cur.append(line); 
            if line.strip().startswith('.size'): name = None
            continue
        cur.append(line)
    return out

def norm(lines):
    res = []
    for l in lines:
        l = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', l)
        l = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', l)
        l = re.sub(r'_Z\S+', 'SYM', l)
        if l.strip().startswith(';'): continue
        l = re.sub(r'\s*;.*$', '', l.rstrip('\n'))
        res.append(l)
    return res

def dem(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, r))

a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
da, db = dem(list(a)), dem(list(b))
ia = {v: k for k, v in da.items()}
same = diff = 0; newonly = []
for nb, d in db.items():
    old = re.sub(r', float>', '>', d)
    old = re.sub(r'<float>', '', old)
    if old in ia:
        if norm(a[ia[old]]) == norm(b[nb]): same += 1
        else:
            diff += 1; print('DIFF', d)
    else:
        newonly.append(d)
unmatched = [da[k] for k in a if da[k] not in {re.sub(r'<float>', '', re.sub(r', float>', '>', x)) for x in db.values()}]
print(f'identical {same}, differ {diff}, new-only {len(newonly)}, old unmatched {len(unmatched)}')
for x in unmatched: print('  OLD-UNMATCHED', x)
if '-v' in sys.argv:
    for x in newonly: print('  NEW', x)
if '--show' in sys.argv:
    import difflib
    tgt = sys.argv[sys.argv.index('--show') + 1]
    for nb, d in db.items():
        if d == tgt:
            old = re.sub(r'<float>', '', re.sub(r', float>', '>', d))
            print(''.join(list(difflib.unified_diff(norm(a[ia[old]]), norm(b[nb]), n=1))[:80]))
