"""Cases for ``ffpa_mla_sparse_topk_slots`` / ``ffpa_mla_sparse_slots`` past one step of the kernel's ordered pass (csrc/ffpa_mla_sparse_topk.hip), with the
conditions that keep each from being vacuous.  No GPU here: a case is a dict of CPU tensors and arguments — ``scores`` or ``positions``, ``topk``,
``cache_seqlens``, ``block_table``, ``page_size``, ``cu_seqlens_q``, ``causal``, ``name`` — plus ``check``, a function of the case that asserts its conditions on
the per-row facts (``facts``).  The facts come from the definition only (tests/kvcache_mla_sparse_topk_ref.py: the stable descending sort), with the selection's
equality: -0.0 == +0.0, all NaNs equal and the largest.  tests/test_kvcache_mla_sparse_topk_cases.py runs every condition on the CPU,
tests/test_kvcache_mla_sparse_topk_sweep_gpu.py runs them again in front of every launch.

What the ordered pass carries from step to step, and the placed group that pins it: ``tie_run`` (step edges, the tie field, ties only behind the first step, the
special tie values), ``need`` (used up on a step's last column, used up in step 0 with the count open until the last step), ``taken_run`` as the base of every
output index (every group with ``topk`` past a step, the positions mode past a step), the early exit (after step 0 / only after the last step), ``par`` (every
case of three or more steps)."""

import torch

import kvcache_mla_sparse_topk_ref as TR

# The kernel's constants: kSpan = kThreads * kPer = 1024 * 8 columns per step of the ordered pass (and per ``base`` of a histogram pass); a wave holds 64 * kPer
# consecutive columns of a step, in kPer pieces of 64 (one ballot each); the translation sweeps kThreads entries at a time.
S, SEG, PIECE, THREADS = 8192, 512, 64, 1024
N3 = 3 * S + 5  # the placed rows: three full steps and five columns of a fourth
NAN, INF = float("nan"), float("inf")
V_TIE, V_BIG = 2.0, 3.0


def keys(x):
  """The kernel's key transform (its header comment), as int64 in [0, 2^32): unsigned order = the selection's order.
    1. -0.0 -> +0.0;
    2. every NaN -> 0xFFFFFFFF;
    3. the sign flip: a negative score's bits are inverted, a positive one's get the top bit."""
  u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
  u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
  k = torch.where((u & 0x80000000) != 0, u ^ 0xFFFFFFFF, u | 0x80000000)
  return torch.where((u & 0x7FFFFFFF) > 0x7F800000, torch.full_like(u, 0xFFFFFFFF), k)


def shared_bytes(a, b):
  """The number of leading bytes two keys share (0 ... 4)."""
  a, b = int(a), int(b)
  return next((k for k in range(4) if (a >> (24 - 8 * k)) & 0xFF != (b >> (24 - 8 * k)) & 0xFF), 4)


def steps(cols):
  """The steps of the ordered pass a list / tensor of columns lies in."""
  return sorted({int(c) // S for c in cols})


def facts(row, n, topk):
  """One score row under visible length ``n``: what the definition selects and why.  ``thr`` the value at rank topk of the stable descending sort, ``larger`` the
  count of strictly larger keys, ``need = topk - larger``, ``ties`` the positions < n equal to ``thr`` (ascending), ``taken`` those of them that are selected,
  ``selected`` the whole selection, ``last`` its last column (-1: empty).  With n <= topk there is no threshold: ``thr`` None, no ties, need 0."""
  n = max(min(int(n), row.numel()), 0)
  selected = TR.select(row, n, topk)
  f = dict(n=n, topk=topk, selected=selected, last=int(selected[-1]) if selected.numel() else -1, thr=None, larger=min(n, topk), need=0,
           ties=torch.empty(0, dtype=torch.int64), taken=torch.empty(0, dtype=torch.int64))
  if n <= topk:
    return f
  vis = row[:n]
  thr = vis[torch.sort(vis, descending=True, stable=True).indices[topk - 1]]
  if torch.isnan(thr):
    equal, larger = torch.isnan(vis), torch.zeros_like(vis, dtype=torch.bool)
  else:
    equal, larger = vis == thr, (vis > thr) | torch.isnan(vis)
  ties = equal.nonzero().flatten()
  chosen = torch.zeros(n, dtype=torch.bool)
  chosen[selected] = True
  f.update(thr=float(thr), larger=int(larger.sum()), ties=ties, taken=ties[chosen[ties]])
  f["need"] = topk - f["larger"]
  # what the definition says about ties, in the words of the kernel: every larger key is selected, and the FIRST `need` ties, no other
  assert 1 <= f["need"] <= ties.numel() and bool(chosen[larger].all()) and torch.equal(f["taken"], ties[: f["need"]]) and selected.numel() == topk
  return f


def visible_lengths(case):
  """Per row of a scores case its visible length, or None for a padding row."""
  scores = case["scores"]
  lens = [int(x) for x in case["cache_seqlens"]]
  rows = TR.token_sequences(scores.size(0), case["cache_seqlens"], case["cu_seqlens_q"])
  return [None if w is None else TR.visible(lens[w[0]], w[2], w[1], scores.size(1), case["causal"]) for w in rows]


def row_facts(case):
  """``facts`` of every row of a scores case (None for a padding row)."""
  return [None if n is None else facts(case["scores"][t], n, case["topk"]) for t, n in enumerate(visible_lengths(case))]


def conditions(case):
  """Assert what keeps the case from being vacuous -> the facts its check computed (or None)."""
  return case["check"](case) if case.get("check") is not None else None


def _i32(x):
  return torch.tensor(x, dtype=torch.int32)


def _case(name, rows, topk, lens=None, table=None, page=None, cu=None, causal=True, check=None, positions=False):
  lens = _i32([rows.size(1)] * rows.size(0)) if lens is None else _i32(lens) if not torch.is_tensor(lens) else lens
  return dict(name=name, scores=None if positions else rows, positions=rows if positions else None, topk=topk, cache_seqlens=lens, block_table=table, page_size=page,
              cu_seqlens_q=cu, causal=causal, check=check)


def shuffled_table(B, W, page, seed, pad=5, spare=9):
  """A shuffled table [B, W] as a view of a wider storage whose other columns lie far outside any pool."""
  store = torch.full((B, W + pad), 2 ** 30, dtype=torch.int32)
  table = store[:, :W]
  table.copy_(torch.randperm(B * W + spare, generator=torch.Generator().manual_seed(seed))[: B * W].view(B, W))
  return table


def padded_rows(rows, pad, fill):
  """``rows`` as a view of a storage ``pad`` columns wider, the other columns holding ``fill``."""
  store = torch.full((rows.size(0), rows.size(1) + pad), fill, dtype=rows.dtype)
  store[:, : rows.size(1)] = rows
  return store[:, : rows.size(1)]


# ============================================================================= the placed cases
def placed_row(ties, larger, seed, N=N3):
  """A background strictly below the tie value (-2 < x <= -1, all different enough not to matter), V_TIE at ``ties``, V_BIG and above at ``larger``."""
  row = -1 - torch.rand(N, generator=torch.Generator().manual_seed(seed))
  row[torch.as_tensor(ties, dtype=torch.int64)] = V_TIE
  big = torch.as_tensor(larger, dtype=torch.int64)
  row[big] = V_BIG + torch.arange(big.numel(), dtype=torch.float32)
  return row


def _placed(name, ties, larger, need, seed, check):
  """One row, topk = L + need; the generic conditions (the ties and the larger keys are the placed ones, `need` is the asked one), then the group's own."""
  ties, larger = sorted(ties), sorted(larger)

  def whole(case):
    f = row_facts(case)[0]
    assert f["thr"] == V_TIE and f["ties"].tolist() == ties and f["larger"] == len(larger) and f["need"] == need and f["taken"].tolist() == ties[:need], name
    check(f)
    return f

  return _case(name, placed_row(ties, larger, seed)[None], len(larger) + need, check=whole)


EDGE_TIES = [S - 1, S, 2 * S - 1, 2 * S, 3 * S, 3 * S + 4]


def step_edges():
  """Ties on both sides of every step edge and in the short last step, one larger key per full step, need = 1 ... 6: `tie_run` carried over one, two and three
  step edges, a tie refused in the step behind the one that used `need` up."""
  def check(need):
    def f_(f):
      assert need < 2 or len(steps(f["taken"])) >= 2, need   # the taken ties lie in two or more steps
      assert need == 6 or f["taken"].numel() < f["ties"].numel(), need  # at least one tie is refused
    return f_
  return [_placed(f"step edges, need {need}", EDGE_TIES, [100, S + 100, 2 * S + 100], need, 11, check(need)) for need in range(1, 7)]


def need_ends_a_step():
  """`need` = 3 used up on the last three columns of step 0, three more ties behind it.  All larger keys in step 0: the count is reached with step 0 and the pass
  must end there.  Then one larger key at the row's last column: the pass walks every step and takes no further tie."""
  ties, big = [S - 3, S - 2, S - 1, S, S + 1, 2 * S + 7], [0, 17, 511, 512, 4000]

  def ends(f):
    assert f["taken"].tolist() == [S - 3, S - 2, S - 1] and f["last"] == S - 1  # taken_run == want at the end of step 0

  def walks(f):
    assert f["taken"].tolist() == [S - 3, S - 2, S - 1] and f["last"] == N3 - 1 and steps(f["selected"]) == [0, 3]

  return [_placed("need ends step 0, the pass ends", ties, big, 3, 12, ends), _placed("need ends step 0, the pass walks on", ties, big + [3 * S + 4], 3, 12, walks)]


def ties_behind_the_first_step():
  """700 larger keys, all in step 0; 40 ties in step 1 and 40 in step 2; need = 55 ends inside step 2."""
  g = torch.Generator().manual_seed(13)
  big = torch.randperm(S, generator=g)[:700].tolist()
  ties = (S + torch.randperm(S, generator=g)[:40]).tolist() + (2 * S + torch.randperm(S, generator=g)[:40]).tolist()

  def check(f):
    assert steps(f["ties"]) == [1, 2] and steps(f["taken"]) == [1, 2] and steps(f["ties"][f["need"]:]) == [2] and max(big) < S and len(big) == 700

  def behind(f):
    check(f)
    assert f["last"] == N3 - 1 and int(f["selected"][-2]) == int(f["taken"][-1])  # (an output index behind the last taken tie: it counts the ties of both steps)

  # the second row is this file's own: with nothing selected behind the ties, a pass that takes too many of step 2's ties stores the right row all the same
  return [_placed("ties only behind the first step", ties, big, 55, 13, check), _placed("ties only behind the first step, a larger key behind them", ties, big + [3 * S + 4], 55, 13, behind)]


def larger_keys_only_in_the_last_step():
  """Ties at every seventh column from column 0; need = 100 is used up in step 0, the four larger keys lie in the short last step: `taken_run` stays below
  `want` until step 3 and every tie of steps 1 ... 3 must be refused."""
  big = [3 * S, 3 * S + 2, 3 * S + 3, 3 * S + 4]  # (3 S + 1 is a multiple of seven: a tie)

  def check(f):
    assert steps(f["taken"]) == [0] and steps(f["ties"]) == [0, 1, 2, 3] and f["last"] == N3 - 1 and int(f["selected"][f["need"] - 1]) < S and int(f["selected"][f["need"]]) == 3 * S

  return [_placed("larger keys only in the last step", list(range(0, N3, 7)), big, 100, 14, check)]


FIELD_BIG = [7, 600, S, 2 * S - 1, 3 * S + 4]
# need -> the boundary it is named for: (unit, the needs on either side).  The unit counts COLUMNS (a piece, a wave's segment, a step) except for "topk", where
# the output count topk = 5 + need stands on either side of S (S - 1, S, S + 1 entries: the translation's eighth sweep ends, the indices pass one step).
FIELD_NEEDS = {1: None, 63: (PIECE, 63, 65), 64: (PIECE, 63, 65), 65: (PIECE, 63, 65), 511: (SEG, 511, 513), 512: (SEG, 511, 513), 513: (SEG, 511, 513),
               S - 6: ("topk", S - 6, S - 4), S - 5: ("topk", S - 6, S - 4), S - 4: ("topk", S - 6, S - 4), S - 3: (S, S - 3, S - 1), S - 2: (S, S - 3, S - 1),
               S - 1: (S, S - 3, S - 1), S + 1: (S, 1, S + 1), 2 * S + 3: (2 * S, S + 1, 2 * S + 3)}


def field_last(need):
  """The column of the need-th tie of the tie field, by counting: the need-th column that holds no larger key."""
  c = need - 1
  for b in FIELD_BIG:  # (ascending: every larger key at or in front of the candidate moves it one column on)
    if b <= c:
      c += 1
  return c


def tie_field():
  """Every column equals the tie value but five larger keys: thousands of ties per step, `need` on either side of a piece's, a wave's and a step's edge (S - 3 ...
  S - 1 put the last taken column on either side of the step edge, S - 6 ... S - 4 the output count on either side of S)."""
  row = torch.full((N3,), V_TIE)
  row[torch.tensor(FIELD_BIG)] = V_BIG

  def check(need):
    def whole(case):
      f = row_facts(case)[0]
      assert f["thr"] == V_TIE and f["larger"] == 5 and f["need"] == need and int(f["taken"][-1]) == field_last(need) and f["ties"].numel() == N3 - 5
      if FIELD_NEEDS[need] is not None:
        unit, lo, hi = FIELD_NEEDS[need]
        if unit == "topk":
          assert 5 + lo < S < 5 + hi and field_last(hi) < S  # the count straddles S inside step 0
        else:
          assert field_last(lo) // unit < field_last(hi) // unit and lo <= need <= hi  # the last taken column straddles the edge
      if need > S:
        assert len(steps(f["taken"])) == (2 if need == S + 1 else 3)
      return f
    return whole

  return [_case(f"tie field, need {need}", row[None], 5 + need, check=check(need)) for need in FIELD_NEEDS]


NAN_AT = [7, 600, S - 1, S, 2 * S - 1, 2 * S, 3 * S, 3 * S + 4, 9000, 20000]
FINITE_AT = [3, 100, S, 2 * S + 1, 3 * S + 4]


def special_rows():
  """The three rows whose tie value is special: ten NaNs on a random background; -inf everywhere but five finite scores, -0.0 and +0.0 among them; a sparse row
  whose zeros carry both signs.  The last is ``relu(randn - 1.5)`` with every third column negated and its first 2048 columns lowered by one: the plain
  ``relu(randn - 1)`` has about 2560 positive entries in 24581, so its rank-2048 threshold is not zero, and its zeros are so dense that S + 1 entries end inside
  step 0."""
  g = torch.Generator().manual_seed(15)
  nans = torch.randn(N3, generator=g)
  nans[torch.tensor(NAN_AT)] = NAN
  few = torch.full((N3,), -INF)
  few[torch.tensor(FINITE_AT)] = torch.tensor([-0.0, 1.5, 0.0, -7.0, 1e-45])
  sparse = torch.relu(torch.randn(N3, generator=g) - 1.5)
  sparse[::3] = -sparse[::3]
  sparse[:2048] -= 1
  return torch.stack([nans, few, sparse])


def special_tie_values():
  rows = special_rows()

  def check(topk):
    def whole(case):
      fs = row_facts(case)
      assert torch.signbit(rows[2][rows[2] == 0]).any() and not torch.signbit(rows[2][rows[2] == 0]).all() and torch.signbit(rows[1, 3]) and rows[1, 3] == 0
      if topk == 3:
        assert fs[0]["selected"].tolist() == [7, 600, 8191]
      if topk <= 10:
        assert fs[0]["thr"] != fs[0]["thr"] and fs[0]["larger"] == 0 and fs[0]["ties"].tolist() == sorted(NAN_AT)  # (NaN is the threshold)
      if topk == 9:
        assert len(steps(fs[0]["taken"])) == 4 and fs[1]["selected"].tolist() == [0, 1, 2, 3, 4, 100, 8192, 16385, 24580]
      if topk >= 9:
        assert fs[1]["thr"] == -INF and fs[1]["larger"] == 5 and len(steps(fs[1]["ties"])) == 4
      if topk in (2048, S + 1):
        assert fs[2]["thr"] == 0 and fs[2]["larger"] < 2048 and torch.signbit(rows[2][fs[2]["taken"]]).any() and not torch.signbit(rows[2][fs[2]["taken"]]).all()
      if topk == S + 1:
        assert len(steps(fs[2]["taken"])) >= 2
      return fs
    return whole

  return [_case(f"special tie values, topk {topk}", rows, topk, check=check(topk)) for topk in (3, 9, 2048, S + 1)]


DEPTH_N = 20000
DEPTH_TOPK = (1, 700, 8193, 19999)


def _split(total, parts):
  return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


def depth_rows():
  """Four rows of 20000 columns (three histogram bases per pass): the keys at ranks topk and topk + 1 first differ in byte k = 1 ... 4, for every topk of
  DEPTH_TOPK, and in the negated rows too.
    k = 4: 1 + i * 2^-23, the bits 0x3F800000 + i;          k = 3: 1 + i * 2^-15, the bits 0x3F800000 + (i << 8);
    k = 2: the bits (0x2000 + i) << 16 (bfloat16 values);   in these three the ranks r and r + 1 share byte k - 1 unless i crosses a multiple of 256;
    k = 1: the bits b << 24 — at most 254 different values, so equal ones repeat, in runs whose ends fall on the ranks 1, 700, 8193 and N minus these: the
           rank's bucket is taken whole in the first pass."""
  g = torch.Generator().manual_seed(16)
  i = torch.arange(DEPTH_N, dtype=torch.int64)
  bits = [None, (0x2000 + i) << 16, 0x3F800000 + (i << 8), 0x3F800000 + i]
  runs = [1] + _split(699, 20) + _split(7493, 40) + _split(3614, 30) + _split(7493, 40) + _split(699, 20) + [1]  # descending values, 152 of them
  top = [b for b in range(0x7F, 0x00, -1)] + [b for b in range(0x81, 0x100)]  # the bytes of descending floats: positive ones down, then negative ones (0x00 / 0x80 are the zeros: left out)
  assert sum(runs) == DEPTH_N and len(runs) <= len(top)
  pick = [top[j * len(top) // len(runs)] for j in range(len(runs))]
  bits[0] = torch.repeat_interleave(torch.tensor(pick, dtype=torch.int64) << 24, torch.tensor(runs))
  rows = [((b + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).view(torch.float32)[torch.randperm(DEPTH_N, generator=g)] for b in bits]
  rows = torch.stack(rows + [-r for r in rows])
  assert torch.isfinite(rows).all()
  return rows


def radix_depth():
  rows = depth_rows()

  def check(topk):
    def whole(case):
      ranked = torch.sort(keys(rows), dim=-1, descending=True).values
      got = [shared_bytes(ranked[r, topk - 1], ranked[r, topk]) for r in range(8)]
      assert got == [0, 1, 2, 3] * 2, (topk, got)  # byte k is the first to differ: the select needs k passes
      return row_facts(case)
    return whole

  return [_case(f"radix depth, topk {topk}", rows, topk, check=check(topk)) for topk in DEPTH_TOPK]


PAST_A_STEP = ((8193, 8192), (8193, 8193), (24581, 8193), (24581, 16384), (24581, 24580), (40000, 12000))


def topk_past_a_step(N, topk):
  """fp32 randn and bf16-rounded randn, lengths [N, topk + 1, topk, topk - 1, 5] in one launch; no table, a shuffled table of page 16 inside a wider storage, a
  table half as wide as the row (the W - 1 clamp)."""
  lens, W = [N, topk + 1, topk, topk - 1, 5], -(-N // 16)
  out = []
  for family in ("fp32", "bf16"):
    rows = torch.randn(5, N, generator=torch.Generator().manual_seed(N + topk))
    rows = rows.bfloat16().float() if family == "bf16" else rows

    def check(case, family=family):
      fs = row_facts(case)
      assert topk >= S and [f["n"] for f in fs] == [N, min(topk + 1, N), topk, topk - 1, 5] and fs[2]["selected"].numel() == topk > 8 * THREADS - 1
      if N > topk:
        assert fs[0]["last"] >= S and fs[0]["thr"] is not None
        if family == "bf16":
          assert topk > N - 1000 or fs[0]["ties"].numel() > 1  # (bf16 rounding leaves equal keys at the threshold)
      return fs

    for how, table in (("no table", None), ("table", shuffled_table(5, W, 16, N)), ("short table", shuffled_table(5, W // 2, 16, N + 1))):
      out.append(_case(f"N {N} topk {topk} {family}, {how}", rows, topk, lens, table, None if table is None else 16, check=check))
  return out


POSITIONS_TOPK = (8192, 8193, 20000)
HOLES = ("front", "middle", "half", "all but the last", "everywhere", "nowhere", "the first S", "the last S")  # rows 0 ... 7


def positions_past_a_step(topk):
  """The positions mode over 1, 2 and 3 steps: eight hole patterns (-1 and -3) on rows 0 ... 7 of a ragged batch whose row 8 is padding; with and without a table."""
  g = torch.Generator().manual_seed(topk)
  page, W = 16, 300
  pos = torch.randint(0, W * page + 40, (9, topk), generator=g, dtype=torch.int32)
  pos[0, : topk // 3] = -1
  pos[1, topk // 3: topk // 2] = -3
  pos[2][torch.rand(topk, generator=g) < 0.5] = -1
  pos[3, :-1] = -3
  pos[4] = -1
  pos[6, :S] = -1
  pos[7, -S:] = -3
  cu, lens = _i32([0, 3, 3, 8]), _i32([5, 5, 5])
  table = torch.randperm(3 * W, generator=g).to(torch.int32).view(3, W)

  def check(case):
    live = (case["positions"] >= 0).sum(-1).tolist()
    assert live[:2] == [topk - topk // 3, topk - (topk // 2 - topk // 3)] and 0.4 * topk < live[2] < 0.6 * topk and live[3:8] == [1, 0, topk, topk - S, topk - S]
    assert topk >= S and int(case["cu_seqlens_q"][-1]) == 8 < case["positions"].size(0)

  return [_case(f"positions, topk {topk}, {how}", pos, topk, lens, tb, pg, cu, check=check, positions=True) for how, tb, pg in (("table", table, page), ("no table", None, None))]


def many_sequences():
  """257 ragged sequences of 0, 1, 2, 3, 0, ... query tokens (a nine-level search over cu_seqlens_q) with five NaN padding rows behind them, causal and not; and
  64 sequences of 4 tokens."""
  g = torch.Generator().manual_seed(17)
  B, N, topk = 257, 1000, 100
  counts = [b % 4 for b in range(B)]
  cu = _i32([0] + torch.tensor(counts).cumsum(0).tolist())
  T = int(cu[-1]) + 5
  scores = torch.randn(T, N, generator=g)
  scores[int(cu[-1]):] = NAN
  lens = torch.randint(0, 1101, (B,), generator=g, dtype=torch.int32)
  lens[1], lens[2], lens[3] = 0, 1100, N  # (sequences of 1, 2 and 3 tokens: an empty one, one past the row, one that ends with it)

  def ragged(case):
    ns = visible_lengths(case)
    assert ns[-5:] == [None] * 5 and ns.count(None) == 5 and len(ns) == 389 and min(ns[:-5]) == 0 and max(ns[:-5]) == N
    assert sum(n > topk for n in ns[:-5]) > 100 and sum(n <= topk for n in ns[:-5]) > 10 and torch.isnan(case["scores"][-5:]).all()

  out = [_case(f"257 ragged sequences, causal {causal}", scores, topk, lens, cu=cu, causal=causal, check=ragged) for causal in (True, False)]
  lens64 = torch.randint(0, 1101, (64,), generator=g, dtype=torch.int32)

  def uniform(case):
    ns = visible_lengths(case)
    assert len(ns) == 256 and len(set(ns[:4])) > 1  # (causal: the four tokens of a sequence see different lengths)

  lens64[0] = 500
  return out + [_case("64 sequences of 4 tokens", torch.randn(256, N, generator=g), topk, lens64, check=uniform)]


def bf16_rounded_32k():
  """What a 16-bit indexer hands over (``.float()``) at N = 32768, topk = 2048, page 64: two sequences of two tokens.  Every row has eight or more keys equal to
  its threshold, over three or more steps, some of them refused; in at least one row the taken ones lie in two or more steps."""
  N, topk, page = 32768, 2048, 64
  scores = torch.randn((4, N), generator=torch.Generator().manual_seed(160)).bfloat16().float()

  def check(case):
    fs = row_facts(case)
    assert all(f["ties"].numel() >= 8 and f["need"] < f["ties"].numel() and len(steps(f["ties"])) >= 3 for f in fs) and any(len(steps(f["taken"])) >= 2 for f in fs)
    return fs

  return _case("bf16-rounded scores, N 32768 topk 2048", scores, topk, [N, 20000], shuffled_table(2, N // page, page, 162, pad=0, spare=3), page, check=check)


def graph_fills():
  """N = 24581, topk = S + 1, two rows seeing 24581 and 9000 columns: what one captured launch is replayed on — the step-edges row (and its mirror image), a
  bf16-rounded row, an all-equal row."""
  N, topk, lens = N3, S + 1, [N3, 9000]
  edges = step_edges()[3]["scores"][0]
  fills = (torch.stack([edges, edges.flip(0)]), torch.randn(2, N, generator=torch.Generator().manual_seed(171)).bfloat16().float(), torch.full((2, N), 0.25))

  def check(k):
    def whole(case):
      fs = row_facts(case)
      assert [f["n"] for f in fs] == lens and all(f["last"] >= S for f in fs)
      assert (fs[0]["last"] >= 2 * S, len(steps(fs[0]["taken"])) >= 2, fs[0]["need"] == topk and fs[1]["last"] == topk - 1)[k]
      return fs
    return whole

  table = shuffled_table(2, -(-N // 16), 16, 170)
  return [_case(f"graph fill {k}", fill, topk, lens, table, 16, check=check(k)) for k, fill in enumerate(fills)]


# group name -> its builder (no arguments) -> a list of cases
PLACED = {
  "step edges": step_edges,
  "need ends a step": need_ends_a_step,
  "ties behind the first step": ties_behind_the_first_step,
  "larger keys only in the last step": larger_keys_only_in_the_last_step,
  "tie field": tie_field,
  "special tie values": special_tie_values,
  "radix depth": radix_depth,
  "many sequences": many_sequences,
}
PLACED.update({f"topk past a step, N {N} topk {topk}": (lambda N=N, topk=topk: topk_past_a_step(N, topk)) for N, topk in PAST_A_STEP})
PLACED.update({f"positions past a step, topk {topk}": (lambda topk=topk: positions_past_a_step(topk)) for topk in POSITIONS_TOPK})


# ============================================================================= the seeded sweep
SEEDS = tuple(range(48))
FAMILIES = ("fp32", "bf16", "fp16", "eighths", "relu", "floor", "equal")
NMAX = 40000


def _near(r, lo, hi):
  """A size in [lo, hi]: anywhere, or within 2 of a multiple of 64, 512, 1024 or 8192 — each as often as the other."""
  kind = r(0, 4)
  if kind == 0:
    return r(lo, hi)
  m = (64, 512, 1024, 8192)[kind - 1]
  return min(max(r(0, hi // m) * m + r(-2, 2), lo), hi)


def values(family, T, N, g):
  x = torch.randn(T, N, generator=g)
  if family == "bf16":
    return x.bfloat16().float()
  if family == "fp16":
    return x.half().float()
  if family == "eighths":
    return (x * 8).round() / 8
  if family == "relu":
    x = torch.relu(x - 1)
    x[:, ::3] = -x[:, ::3]  # (-0.0 among the +0.0, and negatives)
    return x
  if family == "floor":
    for t in range(T):
      x[t, int(torch.randint(0, N + 1, (1,), generator=g)):] = -INF
    return x
  if family == "equal":
    return torch.full((T, N), 0.25)
  return x


def sweep_case(seed):
  """The case of one seed: one launch.  Mode (scores 3 in 4), the value family (in turn), T <= 12, the row, topk, the token layout, the lengths, the table and the
  row strides are drawn by the rules below; a positions case draws its hole density per row."""
  g = torch.Generator().manual_seed(5000 + seed)
  r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
  positions = seed % 4 == 3
  family = None if positions else FAMILIES[(seed - seed // 4) % 7]  # (the scores seeds, counted through: every family five times or more)
  N = _near(r, 1, NMAX)
  kind = r(0, 3)
  topk = min(max((r(1, N), 2048 + r(-2, 2), S + r(-2, 2), N - r(0, 3))[kind], 1), N)
  # the token layout
  B = r(1, 4)
  if r(0, 1):
    counts = [r(0, 3) for _ in range(B)]
    counts[r(0, B - 1)] += 1 if sum(counts) == 0 else 0
    cu, T = _i32([0] + torch.tensor(counts).cumsum(0).tolist()), sum(counts) + min(r(0, 2), 12 - sum(counts))
  else:
    cu, T = None, B * r(1, 12 // B)
  causal = bool(r(0, 1))
  lens = [(topk + r(-2, 2), N + r(-2, 2), N + r(3, 500), r(0, 5), r(0, N))[r(0, 4)] for _ in range(B)]
  lens[r(0, B - 1)] = N + r(0, 3)  # (one sequence sees the whole row, up to what causal takes off)
  name = f"seed {seed}: {'positions' if positions else family} T {T} N {N} topk {topk} B {B} {'ragged' if cu is not None else 'uniform'} causal {causal} lens {lens}"
  # the table: none, or a page size and a width (full, or too short), in a padded storage or not
  page = (None, 1, 16, 48, 64)[r(0, 4)]
  table = None
  reach = N if not positions else NMAX
  if page is not None:
    W = -(-reach // page)
    W = max(W // 2, 1) if r(0, 2) == 0 else W
    table = shuffled_table(B, W, page, seed, pad=r(0, 1) * 3)
    name += f" page {page} W {W}"
  if positions:
    rows = torch.randint(0, reach + 40, (T, topk), generator=g, dtype=torch.int32)
    for t in range(T):
      rows[t][torch.rand(topk, generator=g) < (0.0, 0.1, 0.5, 0.9, 1.0)[r(0, 4)]] = (-1, -3)[r(0, 1)]
    rows = padded_rows(rows, r(0, 1) * r(1, 9), -1)
  else:
    rows = values(family, T, N, g)
    if cu is not None:
      rows[int(cu[-1]):] = NAN  # (padding rows: whatever they hold)
    rows = padded_rows(rows, r(0, 1) * r(1, 9), NAN)
  case = _case(name, rows, topk, lens, table, page, cu, causal, positions=positions)
  case["family"] = family
  return case


def census_of(case):
  """What one sweep case reaches: (mode, family, a row whose ordered pass spans two or more steps, a row whose taken ties span two or more steps, topk > S)."""
  topk = case["topk"]
  if case["positions"] is not None:
    live = TR.token_sequences(case["positions"].size(0), case["cache_seqlens"], case["cu_seqlens_q"])
    return dict(mode="positions", family=None, pass_steps=topk > S and any(w is not None for w in live), tie_steps=False, big_topk=topk > S)
  fs = [f for f in row_facts(case) if f is not None]
  return dict(mode="scores", family=case["family"], pass_steps=any(f["last"] >= S for f in fs), tie_steps=any(len(steps(f["taken"])) >= 2 for f in fs), big_topk=topk > S)
