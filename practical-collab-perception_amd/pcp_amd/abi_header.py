"""Reader of the C ABI headers (include/pcp_hip*.h): constants, structs and prototypes as ctypes tables.

It understands exactly the dialect those headers are written in -- comments, `#define PCP_X <integer>`, anonymous enums with explicit
values, `typedef struct [tag] { scalar / pointer / array / embedded-struct fields } pcp_x_t;` and `ret pcp_name(args);` -- and refuses
everything else with a PcpError that names the header and the declaration: a wrong guess here is a shifted argument at a kernel launch.
Pure Python (re + ctypes); imports neither torch nor the library, so tests can feed it altered header text.
"""
import ctypes
import re


class PcpError(RuntimeError):
    pass


SCALARS = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64,
           'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double}
_POINTEE_ONLY = ('void', 'char', 'uint8_t')          # known type names that may only stand behind a `*`

_INT = r'(?:0[xX][0-9a-fA-F]+|\d+)[uU]?'
_WORD = r'(?!const\b)[A-Za-z_]\w*'
# [const] type [const] {* [const]} [name] [ [len] ]  -- one parameter, field or return type
_DECL = re.compile(r'^(?:const\s+)?(%s)(?:\s+const\b)?\s*((?:\*\s*(?:const\b\s*)?)*)(%s)?\s*(?:\[\s*(\w+)\s*\])?$' % (_WORD, _WORD))
_DECLARATOR = re.compile(r'^((?:\*\s*(?:const\b\s*)?)*)(%s)\s*(?:\[\s*(\w+)\s*\])?$' % _WORD)      # behind a comma: `, *b` / `, c[8]`


class Abi:
    """constants {PCP_X: int}, structs {pcp_x_t: ctypes.Structure class}, prototypes {pcp_name: (restype, [argtypes])}, header order"""

    def __init__(self, address_only=()):
        self.constants, self.structs, self.prototypes, self.address_only = {}, {}, {}, frozenset(address_only)


def read(headers, address_only=()):
    """headers: paths, or (name, text) pairs, in dependency order (a struct is declared before the header that uses it).
    address_only: structs a pointer to which is bound as c_void_p, not POINTER(struct) -- their tables live in device memory, and a
    call passes the table's address"""
    abi = Abi(address_only)
    for h in headers:
        if isinstance(h, str):
            with open(h) as f:
                h = (h, f.read())
        _Reader(abi, h[0]).read(h[1])
    return abi


def _int(text):
    return int(text.rstrip('uU'), 0)


class _Reader:
    def __init__(self, abi, header):
        self.abi, self.header, self.decl = abi, header, ''

    def refuse(self, why):
        raise PcpError('%s: %s in `%s`' % (self.header, why, self.decl if len(self.decl) < 200 else self.decl[:200] + ' ...'))

    def declare(self, table, name, value):
        if name in self.abi.constants or name in self.abi.structs or name in self.abi.prototypes:
            self.refuse('%s is declared twice' % name)
        table[name] = value

    def read(self, text):
        text = re.sub(r'/\*.*?\*/', lambda m: ' ' + '\n' * m.group(0).count('\n'), text, flags=re.S)
        text = re.sub(r'//[^\n]*', '', text)
        lines, cplusplus = [], False
        for line in text.split('\n'):
            s = line.strip()
            if not s.startswith('#'):
                lines.append('' if cplusplus else line)        # the `extern "C" {` / `}` lines are not C
                continue
            self.decl = s
            m = re.match(r'#\s*define\s+(PCP_\w+)(.*)$', s)
            if re.match(r'#\s*ifdef\s+__cplusplus$', s):
                cplusplus = True
            elif re.match(r'#\s*endif', s):
                cplusplus = False
            elif m and m.group(2).strip():                     # `#define PCP_HIP_H` (an include guard) has no value and is skipped
                if not re.match(r'\s+%s\s*$' % _INT, m.group(2)):
                    self.refuse('the value of %s is no integer literal' % m.group(1))
                lines.append('#define %s %s;' % (m.group(1), m.group(2).strip()))      # keeps its place among the declarations
        depth, start, text = 0, 0, '\n'.join(lines)
        for i, ch in enumerate(text):
            depth += (ch == '{') - (ch == '}')
            if ch == ';' and depth == 0:
                self.declaration(' '.join(text[start:i].split()))
                start = i + 1
        self.decl = ' '.join(text[start:].split())
        if self.decl:
            self.refuse('text behind the last declaration')

    def declaration(self, decl):
        self.decl = decl
        m = re.match(r'#define (\w+) (\w+)$', decl)
        if m:
            return self.declare(self.abi.constants, m.group(1), _int(m.group(2)))
        m = re.match(r'enum\s*\{(.*)\}$', decl)
        if m:
            for item in filter(None, (s.strip() for s in m.group(1).split(','))):
                e = re.match(r'(PCP_\w+)\s*=\s*(%s)$' % _INT, item)
                if not e:
                    self.refuse('enumerator `%s` is not PCP_NAME = integer' % item)
                self.declare(self.abi.constants, e.group(1), _int(e.group(2)))
            return None
        m = re.match(r'typedef struct(?:\s+\w+)?\s*\{(.*)\}\s*(pcp_\w+_t)$', decl)
        if m:
            return self.declare(self.abi.structs, m.group(2), self.struct(m.group(2), m.group(1)))
        m = re.match(r'([\w\s*]+?)\b(pcp_\w+)\s*\(([^()]*)\)$', decl)
        if m:
            return self.declare(self.abi.prototypes, m.group(2), self.prototype(m.group(1).strip(), m.group(3).strip()))
        self.refuse('not a #define, anonymous enum, typedef struct or prototype of the ABI dialect')

    def ctype(self, base, stars, by_value_struct=False, returned=False):
        if base not in SCALARS and base not in _POINTEE_ONLY and base not in self.abi.structs:
            self.refuse('unknown type name %s (a struct must be declared before it is used)' % base)
        if not stars:
            if base in SCALARS:
                return SCALARS[base]
            if base in self.abi.structs and by_value_struct:
                return self.abi.structs[base]
            self.refuse('%s by value' % base)
        if returned:
            if base != 'char' or stars != 1:
                self.refuse('a pointer return type other than const char *')
            return ctypes.c_char_p
        if base in self.abi.structs and stars == 1 and base not in self.abi.address_only:
            return ctypes.POINTER(self.abi.structs[base])
        return ctypes.c_void_p

    def struct(self, name, body):
        fields = []
        for line in filter(None, (s.strip() for s in body.split(';'))):
            parts = [p.strip() for p in line.split(',')]
            m = _DECL.match(parts[0])
            if not m or not m.group(3):
                self.refuse('field `%s` is not `type name`, `type *name` or `type name[len]`' % line)
            base, decls = m.group(1), [m.groups()[1:]]
            for p in parts[1:]:
                d = _DECLARATOR.match(p)
                if not d:
                    self.refuse('field `%s` is not `type name`, `type *name` or `type name[len]`' % line)
                decls.append(d.groups())
            for stars, field, length in decls:
                if field in [f[0] for f in fields]:
                    self.refuse('field %s is declared twice' % field)
                t = self.ctype(base, stars.count('*'), by_value_struct=True)
                if length is not None:
                    if not re.match(_INT + '$', length) and length not in self.abi.constants:
                        self.refuse('array length %s is neither a literal nor a PCP_ constant defined earlier' % length)
                    t = t * (self.abi.constants[length] if length in self.abi.constants else _int(length))
                fields.append((field, t))
        if not fields:
            self.refuse('struct %s has no fields' % name)
        return type(name, (ctypes.Structure,), {'_fields_': fields})

    def prototype(self, ret, args):
        m = _DECL.match(ret)
        if not m or m.group(3) or m.group(4):
            self.refuse('return type `%s`' % ret)
        restype = self.ctype(m.group(1), m.group(2).count('*'), returned=True)
        argtypes, names = [], []
        for arg in ([] if args == 'void' else [a.strip() for a in args.split(',')]):
            m = _DECL.match(arg)
            if not m:
                self.refuse('parameter `%s` is not `type name` or `type *name`' % arg)
            base, stars, name, length = m.groups()
            if name is None:
                self.refuse('unnamed parameter `%s`' % arg)
            if length is not None:
                self.refuse('array parameter `%s`' % arg)
            if name in names:
                self.refuse('parameter %s is declared twice' % name)
            names.append(name)
            argtypes.append(self.ctype(base, stars.count('*')))
        return restype, argtypes
