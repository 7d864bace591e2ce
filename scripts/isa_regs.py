"""VGPR / AGPR / SGPR / spill / LDS per kernel from a gfx950 assembly file (hipcc -save-temps).

usage: python scripts/isa_regs.py <file.s> [substring of the demangled name]
       python scripts/isa_regs.py <A.s> <B.s>      only the kernels whose figures differ or that exist on one side only;
                                                    exit status 1 if there is any
Measurement aid: waves per SIMD = min(8, 512 // roundup(vgpr, 8)).
"""
import re,sys,subprocess
def regs(path):
    s=open(path).read()
    blocks=s.split('amdhsa.kernels:')[1]
    rows=[]
    for blk in blocks.split('  - .agpr_count:')[1:]:
        n=re.search(r'\.name:\s+(\S+)',blk).group(1)
        v=re.search(r'\.vgpr_count:\s+(\d+)',blk).group(1)
        sg=re.search(r'\.sgpr_count:\s+(\d+)',blk).group(1)
        sp=re.search(r'\.vgpr_spill_count:\s+(\d+)',blk).group(1)
        ag=blk.split('\n')[0].strip()
        lds=re.search(r'\.group_segment_fixed_size:\s+(\d+)',blk).group(1)
        rows.append((n,v,ag,sg,sp,lds))
    dn=subprocess.run(['c++filt']+[r[0] for r in rows],capture_output=True,text=True).stdout.strip().split('\n')
    return [(re.sub(r'\(.*','',d),r) for d,r in zip(dn,rows)]
def fmt(r): return f'vgpr {r[1]:>4s} agpr {r[2]:>3s} sgpr {r[3]:>3s} spill {r[4]} lds {r[5]}'
def waves(r): return min(8,512//((int(r[1])+7)//8*8)) if int(r[1]) else 8
if len(sys.argv)>2 and sys.argv[2].endswith('.s'):
    a={r[0]:(d,r) for d,r in regs(sys.argv[1])}; b={r[0]:(d,r) for d,r in regs(sys.argv[2])}
    bad=0
    for n in sorted(set(a)|set(b)):
        if n not in a or n not in b:
            d=(a.get(n) or b[n])[0]
            print(f'{d[:80]:80s} only in {sys.argv[1] if n in a else sys.argv[2]}'); bad+=1
        elif a[n][1][1:]!=b[n][1][1:]:
            print(f'{a[n][0][:80]:80s} A: {fmt(a[n][1])} (waves {waves(a[n][1])})\n{"":80s} B: {fmt(b[n][1])} (waves {waves(b[n][1])})'); bad+=1
    print(f'{len(a)} / {len(b)} kernels, {bad} differ')
    sys.exit(1 if bad else 0)
for d,r in regs(sys.argv[1]):
    if len(sys.argv)>2 and sys.argv[2] not in d: continue
    print(f'{d[:80]:80s} {fmt(r)}')
