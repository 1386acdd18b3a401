#!/usr/bin/env python3
"""include/durf_hip.h -> the reference-side ctypes binding (include/durf_ctypes_stub.py) and the copy of it
embedded in INTEGRATION.md, and the product's own table durf_amd/_sigs.py, so that no copy can drift from the header;
include/durf_<name>.h (libdurf_<name>.so, a library of its own) -> durf_amd/_<name>_sigs.py likewise, for every <name> in
durf_amd._lib.SATELLITES:
    python tools/gen_integration_stub.py            # rewrite all
    python tools/gen_integration_stub.py --check    # exit 1 if any is stale (tests/test_host_logic.py)
Every table holds the whole contract of its header: the entry points' argument types (SIGS), every `#define DURF_*` as an int
under its C name, every function-like macro as a function of the same name and parameters, and every `typedef struct ...
durf_*` as a ctypes.Structure (tests/test_headers_host.py holds all of it to the C compiler).
The parser handles exactly the C subset the headers use (scalar / pointer parameters, /* */ comments, integer arithmetic in
macro bodies, the struct declarators listed at struct_fields) and stops with an error on anything else."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from durf_amd._lib import SATELLITES  # noqa: E402  (the import reads no satellite's table: one may be missing or stale)
HDR = os.path.join(ROOT, 'include', 'durf_hip.h')
STUB = os.path.join(ROOT, 'include', 'durf_ctypes_stub.py')
SIGS = os.path.join(ROOT, 'durf_amd', '_sigs.py')          # the product's own binding table (durf_amd/_lib.py)
DOC = os.path.join(ROOT, 'INTEGRATION.md')
BEGIN, END = '<!-- BEGIN GENERATED: tools/gen_integration_stub.py -->', '<!-- END GENERATED -->'

SCALARS = {'int': 'i32', 'float': 'f32', 'size_t': 'u64', 'int32_t': 'i32', 'uint32_t': 'C.c_uint32'}


def ctype_of(param):
    """C parameter declaration -> ctypes spelling used in the stub"""
    p = re.sub(r'\bconst\b', '', param).strip()
    name = re.search(r'(\w+)\s*$', p).group(1)
    t = p[:p.rfind(name)].strip()
    stars = t.count('*')
    base = t.replace('*', '').strip()
    if stars == 0:
        return SCALARS[base], name
    if stars == 1 and base == 'float' and name in ('barf_w', 'mults', 'cams_host', 'times_host', 'sensor_host', 'sweeps_host',
                                                     'to_sensor_host', 'cam_a_host', 'cam_b_host', 'origin_host', 'du_host', 'dv_host', 'dw_host', 'normal_xform_host', 'thresholds_host', 'inv_host'):
        return 'C.POINTER(f32)', name          # HOST float arrays (documented as such in the header)
    if stars == 1 and base == 'size_t':
        return 'C.POINTER(u64)', name          # HOST array (per-segment row capacities)
    if stars == 1 and base == 'int':
        return 'C.POINTER(i32)', name          # HOST array (per-segment rows per ray)
    if stars == 2:
        return 'C.POINTER(vp)', name           # host array of device pointers
    return 'vp', name                          # device pointer / stream


def strip_comments(text):
    return re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)


def parse_header(text=None):
    """-> [(name, restype, [(ctype, param name)...])] in header order"""
    text = open(HDR).read() if text is None else text
    body = strip_comments(text)
    out = []
    for m in re.finditer(r'(?:^|\n)\s*(const char\*|int|unsigned|size_t)\s+(durf_\w+)\s*\(([^;{]*?)\)\s*;', body):
        ret, name, args = m.group(1), m.group(2), ' '.join(m.group(3).split())
        params = [] if args in ('', 'void') else [ctype_of(a) for a in args.split(',')]
        out.append((name, {'const char*': 'C.c_char_p', 'int': 'i32', 'unsigned': 'C.c_uint', 'size_t': 'u64'}[ret], params))
    return out


TOKENS = r'(?:\s*(?:0[xX][0-9a-fA-F]+|\d+|[A-Za-z_]\w*|<<|>>|[-+*/%()|&^~,]))*\s*'


def py_expr(body, known, outer, what):
    """a C integer expression -> the same in Python: `/` becomes `//`, (size_t) casts go, every name must be a parameter or an
    earlier constant / macro of this header (`known`) or a constant of durf_hip.h (`outer`: spelled hip.NAME)"""
    body = re.sub(r'\(\s*size_t\s*\)', '', body).strip()
    if not body or not re.fullmatch(TOKENS, body):
        sys.exit('%s: cannot translate %r' % (what, body))

    def name(m):
        t = m.group(0)
        if t == '/':
            return '//'
        if t in known:
            return t
        if t in outer:
            return 'hip.' + t
        sys.exit('%s: %r is neither a parameter nor an earlier DURF_* constant' % (what, t))
    text = re.sub(r'(?<![\w])[A-Za-z_]\w*|/', name, body)
    try:
        compile(text, what, 'eval')
    except SyntaxError as e:
        sys.exit('%s: %r is not an expression (%s)' % (what, body, e))
    return text


def struct_fields(cname, decls, known, outer, structs):
    """the member declarations of one struct -> [(field, ctypes spelling)] in declaration order.  The declarators that occur:
    `int B, N`, `const float *origins, *directions`, `float* zo`, `float barf_w[10]`, `const float* raw_obj[DURF_MAX_OBJ]`,
    `float level_mults[DURF_FORWARD_MAX_LEVELS][6]`, `durf_forward_args f`.  Any pointer is vp (the wrappers assign addresses)."""
    fields = []
    for decl in decls.split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r'(?:const )?(\w+)\b ?(.*)', decl)
        base = m and m.group(1)
        if not m or not (base in SCALARS or base in structs or base in ('void', 'uint8_t')):
            sys.exit('%s: cannot parse the member %r' % (cname, decl))
        for dec in m.group(2).split(','):
            d = re.fullmatch(r'\s*(\**)\s*(\w+)\s*((?:\[\w+\])*)\s*', dec)
            if not d or (not d.group(1) and base in ('void', 'uint8_t')):
                sys.exit('%s: cannot parse the declarator %r of %r' % (cname, dec, decl))
            t = 'vp' if d.group(1) else SCALARS.get(base, base)
            for i, bound in enumerate(reversed(re.findall(r'\[(\w+)\]', d.group(3)))):
                t = '%s * %s' % (t if i == 0 else '(%s)' % t, py_expr(bound, known, outer, '%s.%s' % (cname, d.group(2))))
            fields.append((d.group(2), t))
    return fields


def parse_items(text, outer=()):
    """-> everything but the functions, in header order: ('const', name, Python literal, C body or None),
    ('macro', name, [parameters], Python expression), ('struct', name, [(field, ctypes spelling)])"""
    body = strip_comments(text)
    found, guard = [], None
    for m in re.finditer(r'^[ \t]*#[ \t]*(\w+)[ \t]*(.*?)[ \t]*$', body, flags=re.M):
        directive, rest = m.groups()
        if directive == 'ifndef' and guard is None:
            guard = rest
        elif directive == 'define':
            d = re.fullmatch(r'(DURF_\w+)(?:\(([^()]*)\))?(?:[ \t]+(.*))?', rest)
            if not d or rest.endswith('\\'):
                sys.exit('cannot parse #define %s' % rest)
            if d.group(3) is None and d.group(2) is None and d.group(1) == guard:
                continue                                   # the include guard
            found.append((m.start(), 'define', d.groups()))
        elif directive not in ('ifndef', 'ifdef', 'endif', 'include'):
            sys.exit('preprocessor directive #%s %s: not handled' % (directive, rest))
    for m in re.finditer(r'\btypedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(durf_\w+)\s*;', body):
        if m.group(1) not in ('', m.group(3)):
            sys.exit('struct %s is typedef\'d %s' % (m.group(1), m.group(3)))
        found.append((m.start(), 'struct', (m.group(3), m.group(2))))
    if len(re.findall(r'\b(?:typedef|struct|union|enum)\b', body)) != 2 * sum(kind == 'struct' for _, kind, _ in found):
        sys.exit('a typedef / struct / union / enum that is not `typedef struct [durf_x] {...} durf_x;`')
    items, known, values, structs = [], set(), {}, set()
    for _, kind, parts in sorted(found):
        if kind == 'struct':
            items.append(('struct', parts[0], struct_fields(parts[0], parts[1], known, outer, structs)))
            structs.add(parts[0])
            continue
        name, params, cbody = parts
        if params is not None:
            params = [p.strip() for p in params.split(',')]
            if not all(re.fullmatch(r'[A-Za-z_]\w*', p) for p in params):
                sys.exit('%s: parameters %r' % (name, params))
            items.append(('macro', name, params, py_expr(cbody or '', known | set(params), outer, name)))
        elif re.fullmatch(r'0[xX][0-9a-fA-F]+|[1-9]\d*|0', cbody or ''):
            values[name] = int(cbody, 0)
            items.append(('const', name, cbody, None))
        else:
            expr = py_expr(cbody or '', known, outer, name)
            if 'hip.' in expr or not set(re.findall(r'[A-Za-z_]\w*', expr)) <= set(values):
                sys.exit('%s: %r is not arithmetic over literals and earlier constants of this header' % (name, cbody))
            values[name] = eval(expr, {'__builtins__': {}}, dict(values))
            items.append(('const', name, str(values[name]), cbody))
        known.add(name)
    return items


def render_items(items):
    """the constants, macros and structs of one header as Python, for a module that has `C` and the vp / i32 / f32 / u64 aliases"""
    L, last = [], None
    for item in items:
        kind, name = item[0], item[1]
        if kind != 'const' or last != 'const':
            L += ['', ''] if L else []
        if kind == 'const':
            L.append('%s = %s' % (name, item[2]) + ('' if item[3] is None else '          # %s' % item[3]))
        elif kind == 'macro':
            L += ['def %s(%s):' % (name, ', '.join(item[2])), '    return %s' % item[3]]
        else:
            L += ['class %s(C.Structure):' % name, '    _fields_ = ['] + ['        (%r, %s),' % f for f in item[2]] + ['    ]']
        last = kind
    return L


def render():
    fns = parse_header()
    L = ['"""ctypes binding of libdurf_hip.so for a reference-side caller -- GENERATED from include/durf_hip.h by',
         'tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite).  All `vp` arguments are',
         'DEVICE pointers of caller-owned buffers except `stream` (hipStream_t); C.POINTER(...) arguments are host',
         'arrays.  Every call is asynchronous on `stream` and returns 0 or an error code (durf_last_error()).  The header\'s',
         'constants and argument structs (every pointer field a vp: assign addresses) come first, under their C names."""',
         'import ctypes as C', '', 'vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t', '', '']
    L += render_items(parse_items(open(HDR).read())) + ['', '', 'def bind(path=\'durf_amd/libdurf_hip.so\'):', '    L = C.CDLL(path)']
    for name, ret, params in fns:
        L.append('    L.%s.restype = %s' % (name, ret))
        args = ', '.join(t for t, _ in params)
        names = ', '.join(n for _, n in params)
        line = '    L.%s.argtypes = [%s]' % (name, args)
        L.append(line)
        if names:
            L.append('    #   (%s)' % names)
    L += ['    return L', '']
    return '\n'.join(L)


def render_sigs(hdr=None, lib='libdurf_hip.so'):
    """the binding table of `lib` from header `hdr` (default: include/durf_hip.h)"""
    text = open(hdr or HDR).read()
    # a satellite header includes durf_hip.h and may use its constants: the table then reads them from durf_amd/_sigs.py
    outer = () if hdr is None else {item[1] for item in parse_items(open(HDR).read()) if item[0] == 'const'}
    items = render_items(parse_items(text, outer))
    L = ['"""Argument types of every entry point of %s, and the constants, macros and structs of its header -- GENERATED from' % lib,
         'include/%s by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""' % os.path.basename(hdr or HDR),
         'import ctypes as C', '']
    if any('hip.' in line for line in items):
        L += ['from . import _sigs as hip', '']
    L += ['vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t', '', 'SIGS = {']
    for name, ret, params in parse_header(text):
        L.append('    %r: (%s, [%s]),' % (name, ret, ', '.join(t for t, _ in params)))
    L += ['}', '', ''] + items + ['']
    return '\n'.join(L)


def doc_with_stub(doc, stub):
    a, b = doc.index(BEGIN), doc.index(END)
    return doc[:a + len(BEGIN)] + '\n```python\n' + stub + '```\n' + doc[b:]


def main():
    stub = render()
    files = {STUB: stub, SIGS: render_sigs()}
    for name in SATELLITES:          # include/durf_<name>.h -> the binding table of libdurf_<name>.so
        files[os.path.join(ROOT, 'durf_amd', '_%s_sigs.py' % name)] = render_sigs(os.path.join(ROOT, 'include', 'durf_%s.h' % name),
                                                                              'libdurf_%s.so' % name)
    doc = open(DOC).read()
    files[DOC] = doc_with_stub(doc, stub)
    if '--check' in sys.argv:
        ok = all(os.path.exists(path) and open(path).read() == text for path, text in files.items())
        if not ok:
            print('stale: run python tools/gen_integration_stub.py')
        sys.exit(0 if ok else 1)
    for path, text in files.items():
        open(path, 'w').write(text)
    print('wrote %s (%d functions) and the block in INTEGRATION.md' % (os.path.relpath(STUB, ROOT), len(parse_header())))


if __name__ == '__main__':
    main()
