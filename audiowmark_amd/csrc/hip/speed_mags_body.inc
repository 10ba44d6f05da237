// body of K13 (speed_mags_kernel, speed_mags_batch_kernel; speed.hip), included into both so that the one-clip kernel is compiled from the
// text it always had: SM_COLS = the column table of this workgroup's entry (a.cols | entries[blockIdx.y].cols)
  __shared__ float2 s_tw[512];
  __shared__ float  s_win[512];
  __shared__ float2 s_x[4][XBUF_ELEMS];
  __shared__ float  s_db[SPEED_TILE * SPEED_NB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SpeedCenterDev cd = a.centers[blockIdx.y];
  const int row0 = blockIdx.x * SPEED_TILE;
  if (row0 >= cd.rows)
    return;
  fft512_load_twiddles (t.tw512, s_tw);
  for (int i = threadIdx.x; i < 512; i += blockDim.x)
    s_win[i] = a.window512[i];
  __syncthreads();

  const int C = a.n_channels;
  const float *sub = a.sub + blockIdx.y * a.sub_stride;
  float2 *xbuf = s_x[wave];
  for (int r = wave; r < SPEED_TILE; r += 4)
    {
      const int row = row0 + r;
      if (row >= cd.rows)
        break;
      const long long pos = (long long) row * 128;
      float acc0 = 0.f, acc1 = 0.f;                            // bands 20 + lane, 84 + lane
      for (int c0 = 0; c0 < C; c0 += 2)
        {
          const bool two = c0 + 1 < C;
          float2 z[8];
          bool nz0 = false, nz1 = false;
#pragma unroll
          for (int j = 0; j < 8; j++)
            {
              const int n = lane + 64 * j;
              const float x0 = sub[(pos + n) * C + c0];
              const float x1 = two ? sub[(pos + n) * C + c0 + 1] : 0.f;
              nz0 |= x0 != 0.f;
              nz1 |= x1 != 0.f;
              z[j] = make_float2 (__fmul_rn (x0, s_win[n]), __fmul_rn (x1, s_win[n]));
            }
          const bool live0 = __any (nz0), live1 = __any (nz1);
          fft512_forward (z, xbuf, s_tw, lane);
          xbuf[0 * 64 + lane] = z[0];
          xbuf[1 * 64 + lane] = z[1];
          xbuf[6 * 64 + lane] = z[6];
          xbuf[7 * 64 + lane] = z[7];
          wave_sync();
#pragma unroll
          for (int part = 0; part < 2; part++)
            {
              const int k = SPEED_MIN_BAND + 64 * part + lane;
              if (k <= 100)
                {
                  const float2 zk = xbuf[zpos (k)], zm = xbuf[zpos (512 - k)];
                  const float2 xa = make_float2 (0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
                  const float2 xb = make_float2 (0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
                  float v = part ? acc1 : acc0;
                  v = __fadd_rn (v, live0 ? db_from_complex (xa) : -96.f);
                  if (two)
                    v = __fadd_rn (v, live1 ? db_from_complex (xb) : -96.f);
                  if (part)
                    acc1 = v;
                  else
                    acc0 = v;
                }
            }
          wave_sync();
        }
      s_db[r * SPEED_NB + lane] = acc0;
      if (lane < SPEED_NB - 64)
        s_db[r * SPEED_NB + 64 + lane] = acc1;
    }
  __syncthreads();

  float2 *mags = a.mags + blockIdx.y * a.mags_center_stride;
  const float *db = s_db + lane * SPEED_NB;                    // this lane's row of the tile
  const bool store = row0 + lane < cd.rows;
  const_uint_ptr cols = (const_uint_ptr) SM_COLS;
  for (int col = __builtin_amdgcn_readfirstlane (wave); col < SPEED_COLS; col += 4)
    {
      unsigned int cw[15];
#pragma unroll
      for (int i = 0; i < 15; i++)
        cw[i] = cols[col * 16 + i];
      float u = 0.f, d = 0.f;
#pragma unroll
      for (int i = 0; i < 30; i++)
        u = __fadd_rn (u, db[(cw[i >> 2] >> (8 * (i & 3))) & 0xff]);
#pragma unroll
      for (int i = 30; i < 60; i++)
        d = __fadd_rn (d, db[(cw[i >> 2] >> (8 * (i & 3))) & 0xff]);
      if (store)
        mags[(long long) col * a.ld + row0 + lane] = make_float2 (u, d);
    }
