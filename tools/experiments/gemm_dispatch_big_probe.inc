// Probe build only (-DANYV2V_EXPERIMENTS, `make -C anyv2v_amd/csrc experiments`): included from gemm_big.hip's big_launch_mode<MODE>() in front of
// the persistent-kernel launch.  Flag bit5 + a workspace: the TRACE instantiation writes 32 s_memtime stamps per block
// (tools/gemm_big_trace.py).  The product library contains none of these instantiations.
            if ((d->flags & ANYV2V_GEMM_PROBE_TRACE) && d->workspace != nullptr && (size_t)grid.x * 32 * sizeof(long long) <= (size_t)d->workspace_bytes) {
                k.trace = (long long*)d->workspace;  // debug: phase timestamps of each block's first tile
                if constexpr (MODE == MODE_LINEAR) {
                    if (geglu)
                        hipLaunchKernelGGL((gemm_big_kernel<3, true, MODE_LINEAR, true>), grid, dim3(512), 0, s, k);
                    else
                        hipLaunchKernelGGL((gemm_big_kernel<3, false, MODE_LINEAR, true>), grid, dim3(512), 0, s, k);
                } else {
                    hipLaunchKernelGGL((gemm_big_kernel<3, false, MODE, true>), grid, dim3(512), 0, s, k);
                }
                return av_launch_status("gemm_big<trace>");
            }
