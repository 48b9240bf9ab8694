"""VGPRs / scratch / static LDS of every kernel in a built library, read from the code-object notes (llvm-readelf --notes on the unbundled
gfx950 code objects, llvm-readobj --notes where the ROCm install has no llvm-readelf; no GPU needed).  The library holds one offload bundle
per translation unit.
usage: python tools/kernel_resources.py [lib.so] [substring ...]          table (substring `scratch`: only kernels with a private segment)
       python tools/kernel_resources.py [lib.so] --isa <substring> [out]   disassembly of the first matching kernel + instruction-class counts
       python tools/kernel_resources.py [lib.so] --digest                  one line per kernel, sorted by mangled name: resources, code size,
                                                                           SHA-256 of the code bytes and of the 64-byte descriptor (two builds
                                                                           hold the same device code when their listings are equal)"""
import collections, hashlib, os, re, struct, subprocess, sys, tempfile

LLVM = '/opt/rocm/lib/llvm/bin/'


def code_objects(lib):
    so = open(lib, 'rb').read()
    out, i = [], 0
    while True:
        i = so.find(b'__CLANG_OFFLOAD_BUNDLE__', i)
        if i < 0:
            return out
        n = struct.unpack_from('<Q', so, i + 24)[0]
        off = i + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from('<QQQ', so, off); off += 24
            t = so[off:off + tl].decode(); off += tl
            if 'gfx950' in t and sz:
                out.append(so[i + o:i + o + sz])
        i += 24


def notes_of(co):
    tool = 'llvm-readelf' if os.path.exists(LLVM + 'llvm-readelf') else 'llvm-readobj'      # the same metadata text from either
    with tempfile.NamedTemporaryFile(suffix='.co') as f:
        f.write(co); f.flush()
        return subprocess.run([LLVM + tool, '--notes', f.name], capture_output=True, text=True, check=True).stdout


def rows_of(co):
    rows = []
    for b in notes_of(co).split('- .agpr_count')[1:]:
        g = lambda k: re.search(r'\.%s:\s+(\S+)' % k, b).group(1)
        rows.append((g('name'), int(g('vgpr_count')), int(g('private_segment_fixed_size')), int(g('group_segment_fixed_size'))))
    return rows


def demangle(names):
    return subprocess.run(['c++filt'] + list(names), capture_output=True, text=True).stdout.split('\n')


def isa(cos, pat, out_path):
    for co in cos:
        rows = rows_of(co)
        for r, d in zip(rows, demangle(r[0] for r in rows)):
            if pat in d:
                with tempfile.NamedTemporaryFile(suffix='.co') as f:
                    f.write(co); f.flush()
                    full = subprocess.run([LLVM + 'llvm-objdump', '-d', f.name], capture_output=True, text=True).stdout
                a = full.index('<%s>:' % r[0])
                m = re.search(r'^[0-9a-f]+ <[^>]+>:', full[a + 10:], re.M)
                txt = full[a:a + 10 + m.start()] if m else full[a:]
                ins = [l.split()[0] for l in txt.split('\n') if re.match(r'^\s+[vs]_|^\s+(ds|global|buffer|scratch|flat)_', l)]
                cls = collections.Counter('mfma' if 'mfma' in i else i.split('_')[0] if i[0] in 'vs' else i.split('_')[0] for i in ins)
                print('%s\n  vgpr %d scratch %d lds %d; %d instructions: %s' % (d.split('(')[0], r[1], r[2], r[3], len(ins), dict(cls)))
                print('  most frequent:', collections.Counter(ins).most_common(24))
                if out_path:
                    open(out_path, 'w').write(txt)
                return
    print('no kernel matches', pat)


def symbols_of(co):
    """name -> (bytes of the symbol) for every sized symbol of an ELF64 code object, through the section that holds its address"""
    shoff, = struct.unpack_from('<Q', co, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', co, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', co, shoff + i * shentsize) for i in range(shnum)]
    tabs = [x for x in secs if x[1] == 2] or [x for x in secs if x[1] == 11]                # SHT_SYMTAB, else SHT_DYNSYM
    out = {}
    for tab in tabs:
        strtab = secs[tab[6]]
        for o in range(tab[4], tab[4] + tab[5], 24):
            name, _, _, shndx, value, size = struct.unpack_from('<IBBHQQ', co, o)
            if not size or not 0 < shndx < shnum or secs[shndx][1] == 8:                    # SHT_NOBITS holds no bytes
                continue
            a = strtab[4] + name
            pos = value - secs[shndx][3] + secs[shndx][4]
            out[co[a:co.index(b'\0', a)].decode()] = co[pos:pos + size]
    return out


def digest(cos):
    lines = []
    for co in cos:
        syms = symbols_of(co)
        for b in notes_of(co).split('- .agpr_count:')[1:]:
            b = '    .agpr_count:' + b
            g = lambda k: re.search(r'^    \.%s:\s+(\S+)' % k, b, re.M).group(1)                 # kernel-level keys (arguments are nested deeper)
            name = g('name')
            code, kd = syms[name], syms[g('symbol')]
            assert len(kd) == 64, (name, len(kd))
            lines.append('%s vgpr %s sgpr %s agpr %s private %s group %s kernarg %s code %d %s kd %s' % (
                name, g('vgpr_count'), g('sgpr_count'), g('agpr_count'), g('private_segment_fixed_size'), g('group_segment_fixed_size'),
                g('kernarg_segment_size'), len(code), hashlib.sha256(code).hexdigest(), hashlib.sha256(kd).hexdigest()))
    print('\n'.join(sorted(lines)))


def main():
    args = sys.argv[1:]
    lib = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'diff-vit_amd', 'csrc', 'libp2vit_hip.so')
    if args and args[0].endswith('.so'):
        lib = args.pop(0)
    cos = code_objects(lib)
    if args and args[0] == '--digest':
        return digest(cos)
    if args and args[0] == '--isa':
        return isa(cos, args[1], args[2] if len(args) > 2 else None)
    print('vgpr scratch lds  kernel')
    for co in cos:
        rows = rows_of(co)
        for r, d in zip(rows, demangle(r[0] for r in rows)):
            d = d.replace('void ', '').split('(')[0]
            if not args or any(p in d for p in args) or (args == ['scratch'] and r[2] > 0):
                print('%4d %7d %6d  %s' % (r[1], r[2], r[3], d))


if __name__ == '__main__':
    main()
