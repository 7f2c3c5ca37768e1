#!/bin/bash
# L2 (TCC) hit rate of the GEMM shapes under the dispatcher's tile order.  usage (on the GPU box): SC_GEMM_KERNEL_MODE=0 bash tools/pmc_gemm.sh "<shapes>" <output directory>
# (the forced column bands this script compared, 69 % -> 8192^3 +20 %: EXPERIMENTS.md old section 3.1; the dispatcher now bands from 16 N-tiles up)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
SHAPES=${1:-"qkv fc1"}
O=${2:?output directory}
timeout 200 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCP_TCC_READ_REQ_sum TCC_EA0_RDREQ_sum --output-format csv -d $O -- python $R/tools/gemm_bench.py $SHAPES > $O.log 2>&1
python - "$O" $SHAPES <<'PY'
import glob,csv,collections,sys
per=collections.defaultdict(list)
for f in glob.glob(sys.argv[1]+'/**/*counter_collection.csv',recursive=True):
    for r in csv.DictReader(open(f)):
        if 'gemm256' in r['Kernel_Name']: per[r['Counter_Name']].append((int(r['Dispatch_Id']),float(r['Counter_Value'])))
shapes=sys.argv[2:]
for i,sname in enumerate(shapes):
    d={c:sum(x[1] for x in sorted(v)[7*i+2:7*i+7])/5 for c,v in per.items()}
    print(f"{sname}: hit {d['TCC_HIT_sum']:.3g} miss {d['TCC_MISS_sum']:.3g} hit-rate {d['TCC_HIT_sum']/(d['TCC_HIT_sum']+d['TCC_MISS_sum']):.3f} tcp->tcc rd {d['TCP_TCC_READ_REQ_sum']:.3g} ea_rd {d.get('TCC_EA0_RDREQ_sum',0):.3g}")
PY
