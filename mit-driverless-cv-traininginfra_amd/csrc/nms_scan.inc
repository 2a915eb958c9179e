// The single-wave greedy scan over the suppression matrix, as text: #include it inside `if (wave == 0) { ... }` of a kernel that has
// `PostSmem sm` (__shared__), `int K` (candidates, sorted), `int W` = ceil(K / 64) and `int lane` in scope.  Bit j of sm.mask[i]: candidate
// j > i leaves once i is kept.  Lane w owns word w of the removed set.  Each 64-candidate word is resolved in registers: lane l holds row
// (64w + l)'s bits for this word, the walk over the 64 bits is scalar (v_readlane).  Kept candidates -> sm.keep[0..sm.count) in visiting
// order.  It is text and not a function because hipcc allocates 39 VGPRs for it in a kernel's body and 128, with spills, for the same
// statements behind a call (inlined or not); one copy of the text keeps the kernels from drifting apart all the same.
  unsigned long long removed = 0;
  int count = 0;
  const int Ku = __builtin_amdgcn_readfirstlane(K);
  for (int w = 0; w < W; ++w) {
    const int il = w * 64 + lane;
    const unsigned long long diag = il < Ku ? sm.mask[il][w] : 0ull;
    const int dlo = (int)(unsigned)diag, dhi = (int)(unsigned)(diag >> 32);
    unsigned long long cur = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(removed >> 32), w) << 32) |
                             (unsigned)__builtin_amdgcn_readlane((int)(unsigned)removed, w);
    const int nb = Ku - w * 64;
    if (nb < 64) cur |= ~0ull << nb;  // past the last candidate
    unsigned long long kept = 0;
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const unsigned long long row = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, t) << 32) | (unsigned)__builtin_amdgcn_readlane(dlo, t);
      const unsigned long long alive = ((cur >> t) & 1ull) - 1ull;  // all ones while candidate t has not been removed
      kept |= (1ull << t) & alive;
      cur |= row & alive;
    }
    if ((kept >> lane) & 1ull) sm.keep[count + __popcll(kept & ((1ull << lane) - 1))] = il;
    count += __popcll(kept);
    if (w + 1 < W && lane > w && lane < W) {  // rows of the kept candidates -> later words; all 64 reads in flight at once
#pragma unroll
      for (int t = 0; t < 64; ++t) removed |= sm.mask[w * 64 + t][lane] & (0ull - ((kept >> t) & 1ull));
    }
  }
  if (lane == 0) sm.count = count;
