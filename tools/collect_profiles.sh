#!/bin/bash
# tools/collect_profiles.sh -- run on the GPU box (via gpurun): kernel-trace stats of the default bench command and PMC passes
# (separate runs, --kernel-trace only, as required on this pool) for the pipeline's kernels.  Outputs under gpurun_out/profiles_raw.
# NOTE: gpurun MERGES gpurun_out/ back into the local copy -- delete the local gpurun_out/profiles_raw before a new collection, otherwise
# tools/make_profile_summary.py averages the counters of old and new builds.
# Every profiled run has a time limit of its own, and the script stops at the first run that fails or times out.
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/profiles_raw
mkdir -p $O
# prof SECONDS LOG rocprofv3-arguments...: one profiled run under its own time limit, output to LOG; a non-zero exit ends the script
prof() {
  local secs=$1 log=$2; shift 2
  timeout -k 10 $secs rocprofv3 "$@" > $log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "collect_profiles: exit $rc in $log"; tail -20 $log; exit $rc; fi
}
# MODE=gs (first argument): only the runs that cover the kernels of gs_raster.hip -- the bench command (all durations), the 3DGS frame at both sizes and the
# 3DGS counter passes; tools/make_profile_summary.py ROUND gs_raster.hip then carries the other kernels' counters over (their sources are unchanged).
# MODE=ngp: the reverse -- everything but the 3DGS-only runs, for a change confined to the InstantNGP sources (tools/make_profile_summary.py ROUND ngp_net.hip).
# MODE=nerf: a change confined to csrc/nerf_net.hip -- the bench command (all durations; no bench leg runs the NeRF block) and the fused NeRF block's own
# trace and counter runs (tools/bench_nerf_fused.py); tools/make_profile_summary.py ROUND nerf_net.hip carries every other kernel's counters over.
# MODE=nerf_train: the trace and counter runs of the block's training path alone (tools/bench_nerf_train.py; no bench command) -- a call of its own after
# MODE=nerf when csrc/nerf_grad.hip or the shared csrc/nerf_net.h changed; then tools/make_profile_summary.py ROUND nerf_net.hip nerf_net.h nerf_grad.hip.
# MODE=nerf_rays: a change confined to csrc/nerf_rays.hip -- the bench command (all durations; no bench leg runs the ray stages) and one trace of
# tools/bench_nerf_rays.py; then tools/make_profile_summary.py ROUND nerf_rays.hip (every other kernel's counters carried over).
# MODE=nerf_input_grad: group 20 (csrc/nerf_input_grad.hip, and what it adds to csrc/nerf_rays.hip) -- no bench command (no bench leg runs these kernels; a call
# of its own after MODE=nerf, which runs it): one trace of tools/bench_nerf_input_grad.py, one of tools/bench_nerf_rays.py (the touched ray stages), and the
# NeRF counter groups on the new launches, each a run of its own; then tools/make_profile_summary.py ROUND nerf_input_grad.hip nerf_rays.hip (plus
# nerf_net.hip nerf_net.h after MODE=nerf and MODE=nerf_train when the shared header moved).
# MODE=gs_features: group 21 (csrc/gs_features.hip, csrc/gs_blend.h; no existing source changes) -- the bench command (all durations; no bench leg runs the feature
# pass), one trace of tools/bench_gs_features.py and three counter groups on the two new launches, each a run of its own; then
# tools/make_profile_summary.py ROUND gs_features.hip gs_blend.h (every other kernel's counters carried over).
# MODE=gs_contrib: group 22 (csrc/gs_contrib.hip; no existing source changes) -- the bench command (all durations; no bench leg runs the contribution pass), one
# trace of tools/bench_gs_contributions.py and three counter groups on the new launch, each a run of its own; then
# tools/make_profile_summary.py ROUND gs_contrib.hip (every other kernel's counters carried over).
# MODE=sparse_adam: group 24 (csrc/adam_rows.hip; no existing source changes) -- the bench command (all durations; no bench leg runs the masked step), one trace of
# tools/bench_sparse_adam.py --profile (1 M Gaussians, ONE known mask: random 20 %) and three counter groups on the new launch, each a run of its own; then
# tools/make_profile_summary.py ROUND adam_rows.hip (every other kernel's counters carried over).
# MODE=bilagrid: group 28 (csrc/bilateral_grid.hip; no existing source changes) -- the bench command (all durations; no bench leg runs the colour correction), one
# trace of tools/bench_bilateral_grid.py --profile (slice and TV, forward and backward, 1297 x 840, 200 grids) and three counter groups on the new launches, each a
# run of its own; then tools/make_profile_summary.py ROUND bilateral_grid.hip (every other kernel's counters carried over).
MODE=${1:-all}
# the full bench command (bench.py --full --steps 20 --warmup 5, every leg): the per-kernel averages of the InstantNGP kernels must agree with the bench line
[ "$MODE" != nerf_train ] && [ "$MODE" != nerf_input_grad ] && prof 900 $O/bench_stats.log --kernel-trace --stats --output-format csv -d $O/bench_stats -- python3 $R/bench.py --full --steps 20 --warmup 5
# the 3DGS kernels at ONE size (the bench command runs 1 M and 6 M Gaussians through the same kernel names)
if [ "$MODE" = nerf ] || [ "$MODE" = all ]; then
prof 300 $O/nerf_stats.log --kernel-trace --stats --output-format csv -d $O/nerf_stats -- python3 $R/tools/bench_nerf_fused.py 5
for set in "GRBM_GUI_ACTIVE SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_VALU_MFMA_BUSY_CYCLES" "TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum GRBM_GUI_ACTIVE" "SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_VALU"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 300 $O/pmcnf_$tag.log --pmc $set --kernel-trace --kernel-include-regex k_nerf --output-format csv -d $O/pmcnf_$tag -- python3 $R/tools/bench_nerf_fused.py 5
done
fi
if [ "$MODE" = nerf_train ] || [ "$MODE" = all ]; then
# the training path of the same block (tools/bench_nerf_train.py): one trace, then the same counter groups, each a run of its own
prof 400 $O/nerf_train_stats.log --kernel-trace --stats --output-format csv -d $O/nerf_train_stats -- python3 $R/tools/bench_nerf_train.py 3
for set in "GRBM_GUI_ACTIVE SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_VALU_MFMA_BUSY_CYCLES" "TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum GRBM_GUI_ACTIVE" "SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_VALU"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 400 $O/pmcnt_$tag.log --pmc $set --kernel-trace --kernel-include-regex "k_nerf_(forward|dgrad|wgrad|wreduce)" --output-format csv -d $O/pmcnt_$tag -- python3 $R/tools/bench_nerf_train.py 3
done
fi
if [ "$MODE" = nerf_rays ]; then
prof 300 $O/nerf_rays_stats.log --kernel-trace --stats --output-format csv -d $O/nerf_rays_stats -- python3 $R/tools/bench_nerf_rays.py 7
fi
if [ "$MODE" = nerf_input_grad ]; then
prof 300 $O/nerf_input_grad_stats.log --kernel-trace --stats --output-format csv -d $O/nerf_input_grad_stats -- python3 $R/tools/bench_nerf_input_grad.py 7
prof 300 $O/nerf_rays_stats.log --kernel-trace --stats --output-format csv -d $O/nerf_rays_stats -- python3 $R/tools/bench_nerf_rays.py 7
for set in "GRBM_GUI_ACTIVE SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_VALU_MFMA_BUSY_CYCLES" "TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum GRBM_GUI_ACTIVE" "SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_VALU"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 300 $O/pmcni_$tag.log --pmc $set --kernel-trace --kernel-include-regex "k_nerf_(input_grad|dir_reduce|positions_bw|integrate_bw)" --output-format csv -d $O/pmcni_$tag -- python3 $R/tools/bench_nerf_input_grad.py 7
done
fi
if [ "$MODE" = gs_features ]; then
prof 400 $O/gs_features_stats.log --kernel-trace --stats --output-format csv -d $O/gs_features_stats -- python3 $R/tools/bench_gs_features.py 9
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 400 $O/pmcgs_feat_$tag.log --pmc $set --kernel-trace --kernel-include-regex "k_render_features" --output-format csv -d $O/pmcgs_feat_$tag -- python3 $R/tools/bench_gs_features.py 9
done
fi
if [ "$MODE" = gs_contrib ]; then
prof 300 $O/gs_contrib_stats.log --kernel-trace --stats --output-format csv -d $O/gs_contrib_stats -- python3 $R/tools/bench_gs_contributions.py 9
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 300 $O/pmcgs_contrib_$tag.log --pmc $set --kernel-trace --kernel-include-regex "k_gs_contributions" --output-format csv -d $O/pmcgs_contrib_$tag -- python3 $R/tools/bench_gs_contributions.py 9
done
fi
if [ "$MODE" = sparse_adam ]; then
prof 300 $O/sparse_adam_stats.log --kernel-trace --stats --output-format csv -d $O/sparse_adam_stats -- python3 $R/tools/bench_sparse_adam.py 21 --profile
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 300 $O/pmcgs_sparse_adam_$tag.log --pmc $set --kernel-trace --kernel-include-regex "k_adam_rows" --output-format csv -d $O/pmcgs_sparse_adam_$tag -- python3 $R/tools/bench_sparse_adam.py 21 --profile
done
fi
if [ "$MODE" = bilagrid ]; then
prof 300 $O/bilagrid_stats.log --kernel-trace --stats --output-format csv -d $O/bilagrid_stats -- python3 $R/tools/bench_bilateral_grid.py --profile
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  prof 300 $O/pmcgs_bilagrid_$tag.log --pmc $set --kernel-trace --kernel-include-regex "k_bilagrid" --output-format csv -d $O/pmcgs_bilagrid_$tag -- python3 $R/tools/bench_bilateral_grid.py --profile
done
fi
if [ "$MODE" = nerf ] || [ "$MODE" = nerf_train ] || [ "$MODE" = nerf_rays ] || [ "$MODE" = nerf_input_grad ] || [ "$MODE" = gs_features ] || [ "$MODE" = gs_contrib ] || [ "$MODE" = sparse_adam ] || [ "$MODE" = bilagrid ]; then
find $O -name "*.db" -delete; find $O -name "*_agent_info.csv" -delete; find $O -path "*_stats/*" -name "*kernel_trace.csv" -delete; du -sh $O; [ -f $O/bench_stats.log ] && tail -5 $O/bench_stats.log
exit 0
fi
if [ "$MODE" != ngp ]; then
prof 300 $O/gs_stats.log --kernel-trace --stats --output-format csv -d $O/gs_stats -- python3 $R/tools/bench_gs.py 1000000 20
prof 300 $O/gs6_stats.log --kernel-trace --stats --output-format csv -d $O/gs6_stats -- python3 $R/tools/bench_gs.py 6000000 5
fi
if [ "$MODE" != gs ]; then
prof 600 $O/train_stats.log --kernel-trace --stats --output-format csv -d $O/train_stats -- python3 $R/tools/bench_train.py 2200 20
# the fused training iteration (nerficg_amd.ngp_trainer): 4 warm-up + 3 x 20 iterations, the next batch marched ahead
prof 600 $O/fused_stats.log --kernel-trace --stats --output-format csv -d $O/fused_stats -- python3 $R/tools/bench_train_fused.py 2200 20 1 0 0 1
fi
for set in "FETCH_SIZE" "WRITE_SIZE" "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum GRBM_GUI_ACTIVE TA_BUSY_avr" "TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum" "SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES"; do
  tag=$(echo $set | tr ' ' '_' | cut -c1-32)
  [ "$MODE" != gs ] && prof 300 $O/pmc_$tag.log --pmc $set --kernel-trace --output-format csv -d $O/pmc_$tag -- python3 $R/tools/bench_query.py 2
  [ "$MODE" != ngp ] && prof 300 $O/pmcgs_$tag.log --pmc $set --kernel-trace --output-format csv -d $O/pmcgs_$tag -- python3 $R/tools/bench_gs.py 1000000 2
  [ "$MODE" != gs ] && prof 300 $O/pmctr_$tag.log --pmc $set --kernel-trace --output-format csv -d $O/pmctr_$tag -- python3 $R/tools/bench_train.py 2200 5
  [ "$MODE" != gs ] && prof 300 $O/pmcfu_$tag.log --pmc $set --kernel-trace --output-format csv -d $O/pmcfu_$tag -- python3 $R/tools/bench_train_fused.py 2200 3 0 0 0 1
done
find $O -name "*.db" -delete; find $O -name "*_agent_info.csv" -delete; find $O -path "*_stats/*" -name "*kernel_trace.csv" -delete; du -sh $O; ls -la $O | head -50; tail -5 $O/bench_stats.log
