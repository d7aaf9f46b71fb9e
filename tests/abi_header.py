"""The one parser of the two C headers (include/ecgvit_hip.h, tools/ecgvit_hip_tools.h) and the one comparison of a ctypes table with them.
A plain module, like gemm_cases.py: tests/test_abi.py holds all of `hip.SIGNATURES`, `hip.GemmDesc` and the tools table to the headers, and the
feature tests call `held` for their own entry points."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ecgvit_hip.h')
TOOLS_HEADER = os.path.join(ROOT, 'tools', 'ecgvit_hip_tools.h')

SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float,
           'double': ctypes.c_double}
FIELD_SCALARS = dict(SCALARS, int32_t=ctypes.c_int32)
DESC = 'ecgvit_gemm_desc'


def code(path):
    """the header without comments and preprocessor lines, white space collapsed"""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    src = re.sub(r'//[^\n]*', ' ', src)
    src = re.sub(r'^[ \t]*#.*$', ' ', src, flags=re.M)
    return ' '.join(src.split())


def _type(decl):
    """'const float *x' -> 'float *'; 'int64_t' -> 'int64_t' (a declarator's type: `const` and the name dropped, one space before each `*`)"""
    words = [w for w in re.findall(r'\w+|\*', decl) if w != 'const']
    return ' '.join(words[:-1] if len(words) > 1 and words[-1] != '*' else words)       # (the last word is the name)


def declarations(path=HEADER):
    """{entry point: (return type, [parameter types])} of every function the header declares"""
    out = {}
    src = re.sub(r'typedef struct \w+ \{.*?\} \w+ ;', ' ', code(path).replace(';', ' ;'))
    for m in re.finditer(r'([\w \*]+?)\b(ecgvit_\w+) ?\(([^()]*)\) ;', src):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        assert name not in out, f'{name} declared twice in {path}'
        out[name] = (_type(ret + ' _'), [] if params in ('', 'void') else [_type(p) for p in params.split(',')])
    return out


def desc_fields(path=HEADER):
    """[(type, name)] of the fields of ecgvit_gemm_desc, in order"""
    body = re.search(r'typedef struct ' + DESC + r' \{(.*?)\} ' + DESC + ' ?;', code(path)).group(1)
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(';'))):
        first, *rest = stmt.split(',')
        base = _type(first).replace(' *', '')                # `const float *scale_a, *scale_b`: the base type, a `*` per declarator
        for d in [first] + [base + ' ' + r for r in rest]:
            out.append((_type(d), re.findall(r'\w+', d)[-1]))
    return out


def accepts(ctype, c, desc_struct=None, scalars=SCALARS, returns=False):
    """whether the ctypes type `ctype` passes a C value of type `c` (as `_type` writes it)"""
    if not c.endswith('*'):
        return ctype is scalars.get(c)
    pointee = c[:-1].strip()
    if pointee == DESC:
        return desc_struct is not None and ctype is ctypes.POINTER(desc_struct)
    if returns and pointee == 'char':
        return ctype is ctypes.c_char_p
    if ctype is ctypes.c_void_p:
        return True
    return isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer) and ctype._type_ is scalars.get(pointee, ())


def mismatches(table, decls, desc_struct=None):
    """every difference between a ctypes table {name: (restype, [argtypes])} and `declarations()`; [] = equal, in both directions"""
    out = [f'{n}: in the table, not declared' for n in table if n not in decls] + [f'{n}: declared, not in the table' for n in decls if n not in table]
    for name in (n for n in table if n in decls):
        (res, args), (ret, params) = table[name], decls[name]
        if not accepts(res, ret, desc_struct, returns=True):
            out.append(f'{name}: returns {ret}, the table says {getattr(res, "__name__", res)}')
        if len(args) != len(params):
            out.append(f'{name}: {len(params)} parameters, the table has {len(args)}')
            continue
        out += [f'{name}: parameter {i} is {p}, the table says {getattr(a, "__name__", a)}' for i, (a, p) in enumerate(zip(args, params))
                if not accepts(a, p, desc_struct)]
    return out


def field_mismatches(fields, decl_fields):
    """every difference between a ctypes Structure's `_fields_` and `desc_fields()`: names, order and types"""
    out = [] if len(fields) == len(decl_fields) else [f'{len(decl_fields)} fields declared, {len(fields)} in _fields_']
    for i, ((name, ctype), (c, cname)) in enumerate(zip(fields, decl_fields)):
        if name != cname or not accepts(ctype, c, scalars=FIELD_SCALARS):
            out.append(f'field {i}: {c} {cname}, _fields_ has {getattr(ctype, "__name__", ctype)} {name}')
    return out


def held(arity, table, desc_struct=None, path=HEADER):
    """a feature test's check of its own entry points {name: number of parameters}: each is declared, with that many parameters, as many as its
    row of `table` has, and the row's types are the declaration's -> the declarations, for equalities between siblings"""
    decls = declarations(path)
    for name, nargs in arity.items():
        assert name in decls, f'{name} is not declared in {os.path.relpath(path, ROOT)}'
        assert len(decls[name][1]) == nargs == len(table[name][1]), (name, nargs, decls[name][1], len(table[name][1]))
    bad = mismatches({n: table[n] for n in arity}, {n: decls[n] for n in arity}, desc_struct)
    assert not bad, bad
    return decls
