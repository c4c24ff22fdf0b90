# per-CU workgroup timelines / phase sums of the early-block kernels (timing build; wg_trace_report / wg_phase_report in mkws_embed_timing.h)
cd $GRAFT_REPO_ROOT
O=gpurun_out/wgtrace; rm -rf $O; mkdir -p $O
MKWS_LIB=$GRAFT_REPO_ROOT/multilingual_kws_amd/lib/libmkws_hip_timing.so timeout 300 python tools/one_fwd.py > $O/out.log 2> $O/err.log; echo "rc=$?"
N=$(grep -n "wg-trace\] block1a" $O/err.log | tail -1 | cut -d: -f1)
tail -n +$N $O/err.log | grep "${WG_FILTER:-wg-trace\|wg-phase\|front-timing\|mid-timing}" | cut -c1-420
