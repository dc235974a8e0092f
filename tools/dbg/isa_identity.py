# Which device functions of two trees are instruction-identical?
#   python tools/dbg/isa_identity.py OLD_DIR NEW_DIR [--rename OLD=NEW ...] unit [unit ...]
# OLD_DIR / NEW_DIR hold unit.s, the device assembly of both trees (hipcc with the Makefile's flags plus -S --cuda-device-only).
# Per unit: the number of device functions before / after, then one 'removed' / 'DIFF' / 'added' line for every function that is
# not instruction-identical (labels and comments stripped).  --rename OLD=NEW (repeatable, applied in order to the OLD tree's text
# only) gives a kernel that was renamed between the trees the name it has in the new one; without it such a kernel shows as a
# 'removed' / 'added' pair.
import argparse,re
def funcs(path, ren):
    s=open(path).read()
    s=re.sub(r'__hip_cuid_[0-9a-f]+','__hip_cuid_X',s)
    for a,b in ren: s=s.replace(a,b)
    d={}
    for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:', s, re.S|re.M):
        body=re.sub(r'\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?','.L',m.group(2))
        body=re.sub(r'[ \t]*;.*','',body)   # (and the padding in front of a comment: it follows the label's width)
        d[m.group(1)]=body
    return d
ap=argparse.ArgumentParser()
ap.add_argument('old_dir'); ap.add_argument('new_dir'); ap.add_argument('units',nargs='+')
ap.add_argument('--rename',action='append',default=[],metavar='OLD=NEW',help='substring of a mangled name in the OLD tree -> its name in the new tree')
args=ap.parse_args()
ren=[tuple(r.split('=',1)) for r in args.rename]
for f in args.units:
    a=funcs('%s/%s.s'%(args.old_dir,f),ren); b=funcs('%s/%s.s'%(args.new_dir,f),[])
    print(f,len(a),len(b))
    for k in a:
        if k not in b: print('  removed',k)
        elif a[k]!=b[k]: print('  DIFF',k,len(a[k]),len(b[k]))
    for k in b:
        if k not in a: print('  added',k)
