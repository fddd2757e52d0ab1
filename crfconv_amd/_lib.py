"""ctypes door onto libcrfconv_amd.so.

include/crfconv_amd.h is the single declaration of the C ABI: SIGNATURES and one ctypes.Structure class per record type
(crf_reduce_job -> ReduceJob, crf_pc_dump_job -> PcDumpJob, ..) are read from it when this module is imported.  A new entry
point or job record is added to the header and to csrc/ only.
include/crfconv_blocks.h, the sliding block split, is a second public header read the same way (BLOCKS_SIGNATURES, BLOCKS_RECORDS),
include/crfconv_block_votes.h, the merge of per-block scores onto the points, a third (VOTES_SIGNATURES, VOTES_RECORDS),
include/crfconv_grid.h, the grid subsampling of ragged batches, a fourth (GRID_SIGNATURES, GRID_RECORDS),
include/crfconv_parts.h, the part IoU of ragged shape batches, a fifth (PARTS_SIGNATURES, PARTS_RECORDS), and
csrc/stream_jobs.h holds the entries only this package calls (INTERNAL_*): tables of their own, so the first header's stay its own.

The library is the product: there is no Python / PyTorch fallback.  If it is missing or a call
fails, an exception is raised -- never a silent slow path.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CRFCONV_LIB') or os.path.join(_HERE, 'libcrfconv_amd.so')      # CRFCONV_LIB: A/B builds of scratch/
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'crfconv_amd.h')
INTERNAL_HEADER_PATH = os.path.join(_HERE, 'csrc', 'stream_jobs.h')        # entries only this package calls: not part of the public ABI
BLOCKS_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'crfconv_blocks.h')      # public: the entries behind crfconv_amd.blocks
VOTES_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'crfconv_block_votes.h')      # public: the entries behind blocks.BlockVotes
GRID_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'crfconv_grid.h')      # public: the entries behind crfconv_amd.grid
PARTS_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'crfconv_parts.h')      # public: the entries behind utils.PartScores


class CrfConvError(RuntimeError):
    pass


_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32,
            'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float,
            'double': ctypes.c_double}
_RECORD = re.compile(r'typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTOTYPE = re.compile(r'([\w\s*]*?)(\w+)\s*\(([^()]*)\)')


def _ctype(base, declarator, where):
    """ctypes type of one declarator (`* const* c`, `deg_hi`) behind the type words `base`."""
    if '*' in declarator or base == ['crf_stream_t']:
        return ctypes.c_void_p
    if len(base) != 1 or base[0] not in _SCALARS:
        raise CrfConvError('include/crfconv_amd.h: type `%s` is outside the dialect in `%s`' % (' '.join(base), where))
    return _SCALARS[base[0]]


def _declaration(text, where):
    """`const float* const* c` / `float deg_lo, deg_hi` -> [(name, ctype), ..]: the type words in front of the first `*` or of the last
    identifier, then one declarator per comma."""
    first, *more = text.split(',')
    m = re.fullmatch(r'\s*([\w\s]+?)(\s+|(?:\s*\*(?:\s*const\b)?)+\s*)(\w+)\s*', first)
    if m is None or not all(re.fullmatch(r'[\s*]*\w+\s*', d) for d in more):
        raise CrfConvError('include/crfconv_amd.h: cannot read `%s` in `%s`' % (' '.join(text.split()), where))
    base = [w for w in m.group(1).split() if w != 'const']
    return [(m.group(3), _ctype(base, m.group(2), where))] + [(d.strip('* \t\n'), _ctype(base, d, where)) for d in more]


def parse_header(text):
    """(functions, records) of the header's text: functions name -> (restype, [argtypes]); records C type name -> [(field, ctype), ..]
    in declaration order.  The dialect is the one listed at the top of include/crfconv_amd.h; anything else raises CrfConvError."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$', ' ', text, flags=re.M)
    text, guards = re.subn(r'extern\s+"C"\s*\{', ' ', text)
    text = re.sub(r'typedef\s+void\s*\*\s*crf_stream_t\s*;', ' ', text)
    text = re.sub(r'\benum\s*\{[^{}]*\}\s*;', ' ', text, count=1)
    records = {}

    def record(m):
        where = 'typedef struct %s' % m.group(2)
        fields = [f for part in m.group(1).split(';') if part.strip() for f in _declaration(part, where)]
        if not m.group(2).startswith('crf_') or m.group(2) in records or not fields:
            raise CrfConvError('include/crfconv_amd.h: bad record `%s`' % where)
        records[m.group(2)] = fields
        return ' '
    text = _RECORD.sub(record, text)
    functions = {}
    *prototypes, rest = text.split(';')
    for proto in prototypes:
        where = ' '.join(proto.split())
        m = _PROTOTYPE.fullmatch(proto.strip())
        if m is None or m.group(2) in functions:
            raise CrfConvError('include/crfconv_amd.h: cannot read the declaration `%s`' % where)
        if ''.join(m.group(1).split()) == 'constchar*':
            restype = ctypes.c_char_p
        else:
            restype = _declaration(m.group(1) + ' ' + m.group(2), where)[0][1]
        params = m.group(3).strip()
        args = [] if params == 'void' else [_declaration(p, where)[0][1] for p in params.split(',')]
        functions[m.group(2)] = (restype, args)
    if rest.split() != ['}'] * guards:
        raise CrfConvError('include/crfconv_amd.h: text left over after its declarations: `%s`' % ' '.join(rest.split()))
    return functions, records


def _read_header(path=HEADER_PATH):
    if not os.path.exists(path):
        raise CrfConvError('%s not found: it is the declaration of the C ABI that crfconv_amd reads at import.' % path)
    with open(path) as f:
        return parse_header(f.read())


def record_class_name(c_name):
    """crf_fold1_bwd_job -> Fold1BwdJob."""
    return ''.join(w[:1].upper() + w[1:] for w in c_name[len('crf_'):].split('_'))


def _tables(path, where, taken=()):
    """(signatures, record classes) of one header: name -> (restype, argtypes), and C record name -> its ctypes.Structure class (also a
    module attribute under its CamelCase name).  A name that a table in `taken` holds already is refused."""
    signatures, fields = _read_header(path)
    records = {c_name: type(record_class_name(c_name), (ctypes.Structure,), {'_fields_': f, '__doc__': '%s of %s.' % (c_name, where)})
               for c_name, f in fields.items()}
    if any((set(signatures) | set(records)) & set(t) for t in taken):
        raise CrfConvError('%s declares a name of another header again' % where)
    globals().update((cls.__name__, cls) for cls in records.values())
    return signatures, records


SIGNATURES, RECORDS = _tables(HEADER_PATH, 'include/crfconv_amd.h')
# the package-internal entries of csrc/stream_jobs.h (LinearJob, MlpStreamBwdJob) and the block split's public header: tables of their own
INTERNAL_SIGNATURES, INTERNAL_RECORDS = _tables(INTERNAL_HEADER_PATH, 'csrc/stream_jobs.h', (SIGNATURES, RECORDS))
BLOCKS_SIGNATURES, BLOCKS_RECORDS = _tables(BLOCKS_HEADER_PATH, 'include/crfconv_blocks.h',
                                            (SIGNATURES, RECORDS, INTERNAL_SIGNATURES, INTERNAL_RECORDS))
VOTES_SIGNATURES, VOTES_RECORDS = _tables(VOTES_HEADER_PATH, 'include/crfconv_block_votes.h',
                                          (SIGNATURES, RECORDS, INTERNAL_SIGNATURES, INTERNAL_RECORDS, BLOCKS_SIGNATURES, BLOCKS_RECORDS))
GRID_SIGNATURES, GRID_RECORDS = _tables(GRID_HEADER_PATH, 'include/crfconv_grid.h',
                                        (SIGNATURES, RECORDS, INTERNAL_SIGNATURES, INTERNAL_RECORDS, BLOCKS_SIGNATURES, BLOCKS_RECORDS,
                                         VOTES_SIGNATURES, VOTES_RECORDS))
PARTS_SIGNATURES, PARTS_RECORDS = _tables(PARTS_HEADER_PATH, 'include/crfconv_parts.h',
                                          (SIGNATURES, RECORDS, INTERNAL_SIGNATURES, INTERNAL_RECORDS, BLOCKS_SIGNATURES, BLOCKS_RECORDS,
                                           VOTES_SIGNATURES, VOTES_RECORDS, GRID_SIGNATURES, GRID_RECORDS))

_lib = None


def load():
    """Loads the shared library (once). Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CrfConvError(
                '%s not found: build it with `make -C crfconv_amd/csrc` (or __graft_entry__.build()). '
                'crfconv_amd has no CPU / PyTorch fallback.' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(INTERNAL_SIGNATURES.items()) + list(BLOCKS_SIGNATURES.items())
                                  + list(VOTES_SIGNATURES.items()) + list(GRID_SIGNATURES.items()) + list(PARTS_SIGNATURES.items())):
            fn = getattr(lib, name)      # AttributeError here == header and library out of sync
            fn.restype = res
            fn.argtypes = args
        if lib.crfconv_abi_version() != 1:
            raise CrfConvError('libcrfconv_amd.so ABI version mismatch')
        _lib = lib
    return _lib


def last_error():
    return load().crfconv_last_error().decode('utf-8', 'replace')


def check(rc, what=''):
    """Raise on a negative status; returns rc otherwise (sizes / counts pass through)."""
    if rc < 0:
        raise CrfConvError('%s failed (%d): %s' % (what or 'libcrfconv_amd call', rc, last_error()))
    return rc


_FN = {}          # name -> bound foreign function (the eager path makes ~300 calls per training step: no lookup chain per call)


def call(name, *args):
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(load(), name)
    rc = fn(*args)
    if rc < 0:
        check(rc, name)
    return rc
