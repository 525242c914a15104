// Probe build only (-DANYV2V_EXPERIMENTS): included from gemm_mfma.hip's mfma_launch_mode<MODE>() in front of the 128-row kernel launch.
// Flag bit5: per-block phase timestamps; flags bits 6-8: K-loop knock-outs (wrong results by design) -- tools/gemm_trace.py.
    if ((d->flags & ANYV2V_GEMM_PROBE_TRACE) && glds && k.splits == 1 && d->workspace != nullptr &&
        (size_t)grid.x * 32 * sizeof(long long) <= (size_t)d->workspace_bytes) {  // debug: per-block phase timestamps
        k.trace = (long long*)d->workspace;
        if (geglu)
            hipLaunchKernelGGL((gemm_mfma_kernel<4, true, true, MODE, true>), grid, dim3(256), 0, s, k);
        else if (plan.nf == 5)
            hipLaunchKernelGGL((gemm_mfma_kernel<5, true, false, MODE, true>), grid, dim3(256), 0, s, k);
        else
            hipLaunchKernelGGL((gemm_mfma_kernel<4, true, false, MODE, true>), grid, dim3(256), 0, s, k);
        return av_launch_status("gemm_mfma<trace>");
    }
    const int ko = (d->flags >> ANYV2V_GEMM_PROBE_KO_SHIFT) & 7;  // debug knock-outs (wrong results by design), NF = 5 plain tiles only
    if (ko >= 2 && ko <= 5 && glds && !geglu && plan.nf == 5 && k.splits == 1) {
        if (ko == 2) hipLaunchKernelGGL((gemm_mfma_kernel<5, true, false, MODE, false, 2>), grid, dim3(256), 0, s, k);
        if (ko == 3) hipLaunchKernelGGL((gemm_mfma_kernel<5, true, false, MODE, false, 3>), grid, dim3(256), 0, s, k);
        if (ko == 4) hipLaunchKernelGGL((gemm_mfma_kernel<5, true, false, MODE, false, 4>), grid, dim3(256), 0, s, k);
        if (ko == 5) hipLaunchKernelGGL((gemm_mfma_kernel<5, true, false, MODE, false, 5>), grid, dim3(256), 0, s, k);
        return av_launch_status("gemm_mfma<knock-out>");
    }
