#!/bin/bash
# Lists VGPR / scratch / occupancy of every alignment kernel instantiation; exits 1 if one of them uses scratch.
cd "$(dirname "$0")/../audio_pattern_discovery_amd/csrc"
for fam in sys sysx wf; do for d in 8 10 13 16 20 26; do
  extra=""; [ "$fam" = "sys" ] && extra="-mllvm -amdgpu-sched-strategy=iterative-ilp"; [ "$fam$d" = "sys13" ] && extra="$extra -mllvm -misched-cluster=false"       # as the Makefile builds it
  [ "$fam" = "sysx" ] && extra="-mllvm -amdgpu-sched-strategy=max-ilp"
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize $extra --cuda-device-only -Rpass-analysis=kernel-resource-usage -DAPD_DIM=$d -c dtw_${fam}.hip -o /dev/null 2>&1 \
   | grep -E "Function Name|VGPRs:|ScratchSize|Occupancy" | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' | paste - - - - \
   | sed -E 's/Function Name: _ZN3apd18dtw_fused_systolicILi([0-9]+)ELi([0-9]+)ELi([0-9]+)ELb([01])ELb([01])EEEvNS_11AlignLaunchE/systolic D=\1 C=\2 G=\3 uniform=\4 hybrid=\5/; s/Function Name: _ZN3apd25dtw_fused_systolic_sharedILi([0-9]+)ELi([0-9]+)ELi([0-9]+)EEEvNS_11AlignLaunchE/systolic shared columns D=\1 C=\2 G=\3 (dynamic LDS: shared_columns_lds_bytes, <= 80 KB by static_assert)/' > /tmp/apd_res_${fam}_$d.txt &
done; done
# the UPGMA / companion kernels too: a launch that needs scratch pays for it every time, and the UPGMA loop is made of short launches
# (round 4: two debug stamps in the commit pushed upgma_segment_kernel to 400 bytes of scratch per lane and doubled every dendrogram)
# clustering also holds the medoid kernels (medoid_cost_kernel, medoid_pick_kernel), dtw_path the barycenter kernels (bary_init_kernel,
# bary_scores_kernel, bary_accumulate_kernel, bary_finalize_kernel, bary_pack_kernel)
for unit in clustering companions dtw_path dtw_spot dtw_spot_detect dtw_spot_quantile dtw_spot_online dtw_spot_path dtw_spot_stream dtw_spot_stream_rec; do   # dtw_spot_detect: marking, picking, hit offsets and emit of apd_spot_detect; dtw_spot_quantile: the digit pass and the digit step of apd_spot_quantiles' radix select; dtw_spot_online: the hold-off scan of an armed streaming session and its flush / reset; dtw_path: the warping-path sweep and trace; the four sweep units each list spot_kernel<Kind, rows per lane in registers (0: LDS), D> (dtw_spot_sweep.h) for their kind: dtw_spot: SpotSweep; dtw_spot_path: SpotRecordSweep (the recording sweep) and the window trace dtw_spot_trace; dtw_spot_stream: SpotStreamSweep (carried column) and the session's reset; dtw_spot_stream_rec: SpotStreamRecordSweep (records into a session's rings), the frame-ring copy and the ring trace dtw_spot_stream_trace
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize --cuda-device-only -Rpass-analysis=kernel-resource-usage -c $unit.hip -o /dev/null 2>&1 \
   | grep -E "Function Name|VGPRs:|ScratchSize|Occupancy" | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' | paste - - - - > /tmp/apd_res_${unit}_0.txt &
done
wait
cat /tmp/apd_res_*_*.txt
if grep -v "ScratchSize \[bytes/lane\]: 0" /tmp/apd_res_*_*.txt | grep -q Scratch; then echo "SCRATCH IN USE"; exit 1; fi
echo "no scratch"
