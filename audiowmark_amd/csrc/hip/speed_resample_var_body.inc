// body of K12 (resample_var_kernel, resample_var_batch_kernel; speed.hip), included into both so that the one-clip kernel is compiled
// from the text it always had: RV_IN = the input of this workgroup's entry (a.in | entries[blockIdx.y].in)
  extern __shared__ float s_tab[];                           // lds_floats: sized for the largest table of the launch (occupancy); then the window
  const SpeedCenterDev cd = a.centers[blockIdx.y];
  if ((long long) blockIdx.x * tiles_per_wg * RV_TILE >= cd.n_out)
    return;
  const int stride = cd.stride, n_tab = 257 * stride;
  const bool in_lds = n_tab <= a.lds_floats;
  const bool staged = CT == 2 && in_lds && in_span > 0;
  float2 *s_in = reinterpret_cast<float2 *> (s_tab + ((a.lds_floats + 1) & ~1));
  if (in_lds)
    for (int i = threadIdx.x; i < n_tab; i += blockDim.x)
      s_tab[i] = cd.ctab[i];
  float *out = a.out + blockIdx.y * a.out_stride;
  for (int t = 0; t < tiles_per_wg; t++)
    {
      const long long tile0 = ((long long) blockIdx.x * tiles_per_wg + t) * RV_TILE;
      if (tile0 >= cd.n_out)
        break;                                                                 // (uniform)
      long long first0 = 0;
      if (staged)
        {
          first0 = var_phase (cd, tile0).first;                                // window starts do not decrease with m
          if (t)
            __syncthreads();                                                   // the previous tile's windows have been read
          const float2 *in2 = reinterpret_cast<const float2 *> (RV_IN);
          for (int i = threadIdx.x; i < in_span; i += 256)
            {
              const long long j = first0 + i;
              s_in[i] = (j >= 0 && j < cd.n_in) ? in2[j] : make_float2 (0.f, 0.f);
            }
        }
      if (in_lds && (staged || t == 0))
        __syncthreads();
      for (int q = 0; q < RV_TILE / 256; q++)
        {
          const long long m = tile0 + q * 256 + threadIdx.x;
          if (m >= cd.n_out)
            break;
          if (staged)
            {
              const VarPhase v = var_phase (cd, m);
              const long long rel = v.first - first0;
              if (rel >= 0 && rel + 2 * cd.hl <= in_span)                      // (always, by the launcher's bound; kept as a guard)
                var_output_staged (cd, s_tab, stride, v, s_in + rel, m, out);
              else
                var_output<CT> (cd, s_tab, stride, RV_IN, a.n_channels, m, out);
            }
          else if (in_lds)                                       // two copies of the loop: ds_read vs global_load addressing
            var_output<CT> (cd, s_tab, stride, RV_IN, a.n_channels, m, out);
          else
            var_output<CT> (cd, cd.ctab, stride, RV_IN, a.n_channels, m, out);
        }
    }
