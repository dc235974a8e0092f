import re,sys
def funcs(path, ren):
    s=open(path).read()
    s=re.sub(r'__hip_cuid_[0-9a-f]+','__hip_cuid_X',s)
    for a,b in ren: s=s.replace(a,b)
    s=re.sub(r'(k_gemmILi\d+ENS_7TileCfgILi\d+ELi\d+ELi\d+ELi\d+EEE)Li0E',r'\1',s)   # k_gemm<EPI, T, 0> is k_gemm<EPI, T> of before the MFMA shape parameter
    d={}
    for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:', s, re.S|re.M):
        body=re.sub(r'\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?','.L',m.group(2))
        body=re.sub(r'[ \t]*;.*','',body)   # (and the padding in front of a comment: it follows the label's width)
        d[m.group(1)]=body
    return d
# renames, applied in order to the FIRST (older) tree only: its name -> the name the kernel has in the second tree
ren=[('k_attention_fwdILb0ELb0ELb0ELb0EE','k_attention_fwdILb0ELb0ELb0EE'),('k_attention_fwdILb0ELb0ELb1ELb1EE','k_attention_fwdILb0ELb1ELb1EE'),
     ('k_attention_fwdILb1ELb0ELb0ELb0EE','k_attention_fwdILb1ELb0ELb0EE'),('k_attention_fwdILb1ELb0ELb0ELb1EE','k_attention_fwdILb1ELb0ELb1EE'),
     ('15k_gemm_resid_lnE','24k_gemm_resid_ln_32x32x16E'),   # the retired 32x32x16 kernel steps aside (it shows as removed) ...
     ('19k_gemm_resid_ln_m16E','15k_gemm_resid_lnE')]        # ... for the 16x16x32 kernel that took its name
for f in sys.argv[3:]:
    a=funcs('%s/%s.s'%(sys.argv[1],f),ren); b=funcs('%s/%s.s'%(sys.argv[2],f),[])
    print(f,len(a),len(b))
    for k in a:
        if k not in b: print('  removed',k)
        elif a[k]!=b[k]: print('  DIFF',k,len(a[k]),len(b[k]))
    for k in b:
        if k not in a: print('  added',k)
