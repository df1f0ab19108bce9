#!/usr/bin/env python3
"""Per-kernel assembly of two builds, compared kernel by kernel (instructions and .amdhsa metadata; comments, label numbers and
symbol names normalised).  Kernels are matched by their demangled names.  Prints the kernels that differ and a count line.

    python tools/cmp_kernel_asm.py OLD.s NEW.s [-v] [--show 'demangled kernel name']     (hipcc --save-temps=obj leaves <unit>-hip-amdgcn-amd-amdhsa-gfx950.s)
    python tools/cmp_kernel_asm.py --trees OLD_TREE NEW_TREE SCRATCH_DIR
--trees: every file of build.SOURCES of each tree compiled as build.py compiles it (this tree's build.EXTRA_FLAGS, at most 8 compilations
at a time) into SCRATCH_DIR/old and /new, one count line per translation unit (a unit that OLD does not have is named as new); exit status 1 if any unit has differ, new-only or old unmatched above 0.
--mnemonics (either mode): the opcode sequences only -- operands and .amdhsa metadata dropped (for a change that moves kernel-argument
offsets; tools/kres.py compares registers, spills, scratch and LDS).
--rename 'REGEX=>REPL' (either mode, repeatable, applied in order to OLD's demangled names before matching): for a change that renames
kernels or alters their template or argument lists.
"""
import concurrent.futures, difflib, importlib.util, os, re, subprocess, sys

def funcs(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\S+):\s*(;.*)?$', line)
        if m and not line.startswith('.'):
            name = m.group(1); cur = []; out[name] = cur; continue
        if name is None: continue
        cur.append(line)
        if line.strip().startswith('.size'): name = None
    return out

def norm(lines):
    res = []
    for l in lines:
        l = re.sub(r'_Z\S+', 'SYM', re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', l)))
        if l.strip().startswith(';'): continue
        l = re.sub(r'\s*;.*$', '', l.rstrip('\n'))
        if MNEMONICS:
            if not l.strip() or (l.lstrip().startswith('.') and not l.startswith('.LBB')): continue   # directives, metadata
            l = l.split()[0]
        res.append(l)
    return res

def dem(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, r))

def compare(old_s, new_s, label=''):   # prints the differing kernels and the count line; returns differ + new-only + old unmatched
    a, b = funcs(old_s), funcs(new_s)
    da, db = dem(list(a)), dem(list(b))
    for pat, repl in RENAME: da = {k: re.sub(pat, repl, v) for k, v in da.items()}
    ia = {v: k for k, v in da.items()}
    same, diff, newonly = 0, 0, []
    for nb, d in db.items():
        if d not in ia: newonly.append(d)
        elif norm(a[ia[d]]) == norm(b[nb]): same += 1
        else:
            diff += 1; print('DIFF', d)
            if SHOW == d: print('\n'.join(list(difflib.unified_diff(norm(a[ia[d]]), norm(b[nb]), n=1, lineterm=''))[:80]))
    unmatched = [d for d in da.values() if d not in set(db.values())]
    print(f'{label}identical {same}, differ {diff}, new-only {len(newonly)}, old unmatched {len(unmatched)}')
    for x in unmatched: print('  OLD-UNMATCHED', x)
    if '-v' in sys.argv:
        for x in newonly: print('  NEW', x)
    return diff + len(newonly) + len(unmatched)

def compile_unit(build, tree, out, src):   # as build.build() compiles it, plus --save-temps=obj; returns the device .s
    os.makedirs(out, exist_ok=True)
    csrc, unit = os.path.join(tree, 'egt_amd', 'csrc'), src[:-len('.hip')]
    cmd = [build._hipcc(), f'--offload-arch={build.ARCH}', '-O3', '-std=c++17', '-fPIC', '-c', os.path.join(csrc, src), '-o', os.path.join(out, unit + '.o'),
           '-I', csrc, '-I', os.path.join(tree, 'include'), '-Wno-unused-result', '--save-temps=obj'] + build.EXTRA_FLAGS.get(src, [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0: raise RuntimeError(f'hipcc failed on {tree}: {src}\n{r.stdout}')
    return os.path.join(out, f'{unit}-hip-amdgcn-amd-amdhsa-{build.ARCH}.s')

argv = sys.argv[1:]
MNEMONICS, SHOW = '--mnemonics' in argv, argv[argv.index('--show') + 1] if '--show' in argv else None
RENAME = [argv[i + 1].split('=>') for i, x in enumerate(argv) if x == '--rename']
pos = [x for i, x in enumerate(argv) if not x.startswith('-') and (i == 0 or argv[i - 1] not in ('--show', '--rename'))]
if '--trees' not in argv: compare(pos[0], pos[1])
else:
    spec = importlib.util.spec_from_file_location('egt_build', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'egt_amd', 'build.py'))
    build = importlib.util.module_from_spec(spec); spec.loader.exec_module(build)
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        have = lambda t, s: os.path.exists(os.path.join(t, 'egt_amd', 'csrc', s))
        asm = {(d, s): pool.submit(compile_unit, build, os.path.abspath(t), os.path.join(pos[2], d), s) for t, d in ((pos[0], 'old'), (pos[1], 'new')) for s in build.SOURCES if have(t, s)}
        bad = 0
        for s in build.SOURCES:
            if ('old', s) in asm: bad += compare(asm['old', s].result(), asm['new', s].result(), label=f'{s[:-4]}: ')
            else: print(f"{s[:-4]}: a new translation unit (not in OLD): {len(funcs(asm['new', s].result()))} kernels and device functions, nothing to compare")
    sys.exit(1 if bad else 0)
