"""Compare two device-assembly files (hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --offload-device-only -S) function by function.

    python tools/compare_device_code.py parent.s tree.s

For every function symbol (kernels and the device functions the compiler kept out of line) the instruction text between its label and its
``.Lfunc_end`` is compared after local labels (``.LBB12_3``, ``.Ltmp5``, ``.Lfunc_end7`` ...) are renumbered in order of appearance --
adding a function to the translation unit shifts those numbers and nothing else.  Comment-only lines (``;``) are dropped.  Prints the
functions that exist on one side only, the functions whose code differs (with the first differing line) and a count of identical ones; the
``.amdhsa_`` kernel-descriptor lines of each kernel are compared as well."""
import re
import sys


def functions(path):
    funcs, desc, name, body = {}, {}, None, []
    label = re.compile(r'^([A-Za-z_][\w$.]*):')
    kd = None
    for line in open(path, errors='replace'):
        line = line.rstrip('\n')
        s = line.strip()
        if s.startswith('.amdhsa_kernel '):
            kd = s.split()[1]
            desc[kd] = []
            continue
        if s == '.end_amdhsa_kernel':
            kd = None
            continue
        if kd is not None:
            desc[kd].append(s)
            continue
        m = label.match(line)
        if m and not m.group(1).startswith('.L') and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if s.startswith('.Lfunc_end'):
                funcs[name] = body
                name = None
                continue
            if not s or s.startswith(';') or s.startswith('.p2align') or s.startswith('.loc') or s.startswith('.file') or s.startswith('.cfi'):
                continue
            body.append(s.split(' ; ')[0].rstrip() if ' ; ' in s else s)
    return funcs, desc


def normalise(body):
    ids = {}

    def sub(m):
        return ids.setdefault(m.group(0), f'.L{len(ids)}')
    return [re.sub(r'\.L[A-Za-z_]+\d+(?:_\d+)?', sub, ln) for ln in body]


def main(a, b):
    fa, da = functions(a)
    fb, db = functions(b)
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    same, diff = 0, []
    for name in sorted(set(fa) & set(fb)):
        x, y = normalise(fa[name]), normalise(fb[name])
        if x == y:
            same += 1
        else:
            i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            diff.append((name, len(x), len(y), i, x[i] if i < len(x) else '<end>', y[i] if i < len(y) else '<end>'))
    kd_diff = [k for k in sorted(set(da) & set(db)) if da[k] != db[k]]
    print(f'functions: {len(fa)} in {a}, {len(fb)} in {b}; identical {same}, different {len(diff)}, only in first {len(only_a)}, only in second {len(only_b)}')
    for n in only_a:
        print('only in first :', n)
    for n in only_b:
        print('only in second:', n)
    for name, la, lb, i, p, q in diff:
        print(f'DIFFERENT {name}: {la} / {lb} lines, first difference at line {i}:\n    {p}\n    {q}')
    print(f'kernel descriptors: {len(set(da) & set(db))} common, {len(kd_diff)} different')
    for k in kd_diff:
        changed = [(p, q) for p, q in zip(da[k], db[k]) if p != q]
        print(f'DESCRIPTOR {k}: ' + '; '.join(f'{p} -> {q}' for p, q in changed[:6]))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
