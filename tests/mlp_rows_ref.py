"""CPU side of tests/test_gpu_mlp_edges.py: the base rows of the fused MLP launches and their float64 oracle.

An MLP row depends on no other row, so a launch of any size can be filled with copies of a few base rows and held to the
base launch bit for bit; only the base rows need a reference.  They are RAYS = 16 rays x N = 32 samples (one ray = one
32-row tile) plus RAYS tail rows: the constant encoding [0 x 30, 1 x 30] of a zero-masked Gaussian with each base ray's
view direction -- what a de-duplicated box-hit ray feeds the background MLP (docs/history.md 4.1c).

Forward oracle: oracle.durf_ref.mlp_apply_bf16 in float64 (`forward64` restates it to expose the stashed activations; the
CPU test holds the two equal).  Backward oracle (`backward64`): a float64 restatement of what k_mlp_bwd documents, with
these roundings to bf16 (RNE) and no others -- products and sums are float64 where the kernel accumulates in fp32:
  * the head gradients d raw (csrc/mlp_bwd.hip:497-501: `g10`, `gd`; the same values are dz_out slots 0-3, :502);
  * every kernel, as the packer stores it (csrc/mlp_pack.h:121);
  * every pre-activation gradient where the kernel packs it for the next stage / stores it (bpack_tile, mlp_bwd.hip:45-63):
    dZ of the view layer (:516), of the trunk layers 7..0 (:520-534), and the gradient of the LINEAR bottleneck (:518),
    which is rounded but neither masked nor stored (docs/history.md 4.1e);
  * each masked by the forward's ReLU pattern "stashed bf16 activation != 0" (pack_tile, csrc/mlp_fwd.hip:104-121);
  * d_enc = the skip connection's rows of Dense_5 (:528) + Dense_0 (:541) applied to the ROUNDED dZ5 / dZ0, summed
    unrounded (fp32 in the kernel, :121-122) and stored as fp32 (:542-551).
"""
import torch

from oracle import durf_ref as R

N = 32
RAYS = 16
ROWS = RAYS * N
IN_DIM = {256: 60, 128: 63}
# chosen seeds: the first tried for each width; tests/test_mlp_rows_ref.py holds the conditions below for them
SEEDS = {256: 11, 128: 12}
STASHED = (0, 1, 2, 3, 4, 5, 6, 7, 9)     # stash / dz regions the kernels write (8 = the linear bottleneck: never stored)


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def ident(x):
    return x


def cfg_of(width):
    return R.MLP_BKGD if width == 256 else R.MLP_BOX


def make_base(width):
    """seeded weights (as tests/test_gpu_stages.py::test_mlp_fwd makes them), bf16-representable encodings / view
    directions, head gradients of the base rows and (summed per ray) of the tail rows"""
    in_dim = IN_DIM[width]
    g = torch.Generator().manual_seed(SEEDS[width])
    params, flat = [], []
    for fi, fo in R.mlp_layer_shapes(in_dim, 27, cfg_of(width)):
        lim = (6.0 / (fi + fo)) ** 0.5
        k = (torch.rand(fi, fo, generator=g) * 2 - 1) * lim
        bb = (torch.rand(fo, generator=g) - 0.5) * 0.2
        params.append([k, bb])
        flat += [k.reshape(-1), bb]
    x = torch.randn(RAYS, N, in_dim, generator=g).to(torch.bfloat16).float()
    cond = torch.randn(RAYS, 27, generator=g).to(torch.bfloat16).float()
    draw = torch.randn(ROWS, 4, generator=g) * 0.1
    draw_tail = torch.randn(RAYS, 4, generator=g) * 0.1 * N ** 0.5      # a ray's N head gradients summed
    x_tail = torch.zeros(RAYS, 1, in_dim)
    x_tail[:, :, 30:60] = 1.0
    return dict(width=width, in_dim=in_dim, params=params, flat=torch.cat(flat), x=x, cond=cond, draw=draw,
                draw_tail=draw_tail, x_tail=x_tail)


def forward64(params, x, cond, rnd=bf):
    """x [rows, in_dim], cond [rows, 27] (one view direction per ROW) -> raw [rows, 4] = (rgb, density) and the stashed
    activations, all float64.  rnd = bf: oracle.durf_ref.mlp_apply_bf16; rnd = ident: oracle.durf_ref.mlp_apply."""
    p = [(k.double(), b.double()) for k, b in params]
    x = rnd(x.double())
    inputs, h = x, []
    for i in range(8):
        x = rnd(torch.relu(x @ rnd(p[i][0]) + p[i][1]))
        h.append(x)
        if i == 4:
            x = torch.cat([x, inputs], -1)
    dens = h[7] @ rnd(p[8][0]) + p[8][1]
    bott = rnd(h[7] @ rnd(p[9][0]) + p[9][1])
    hc = rnd(torch.relu(torch.cat([bott, rnd(cond.double())], -1) @ rnd(p[10][0]) + p[10][1]))
    rgb = hc @ rnd(p[11][0]) + p[11][1]
    return dict(raw=torch.cat([rgb, dens], -1), h=h, hc=hc)


def backward64(params, fwd, draw, rnd=bf):
    """-> dz {region: [rows, features]} (regions STASHED: 0..7 the trunk layers, 9 the view layer), d_enc [rows, 64],
    dz_out [rows, 4]: the module docstring lists the roundings.  rnd = ident: the exact reverse mode of forward64(ident)."""
    K = [rnd(k.double()) for k, _ in params]
    W = K[1].shape[0]
    h, hc = fwd['h'], fwd['hc']
    g = rnd(draw.double())
    dz = {9: rnd((g[:, :3] @ K[11].T) * (hc != 0))}
    d_bott = rnd(dz[9] @ K[10][:W].T)
    dz[7] = rnd((d_bott @ K[9].T + g[:, 3:4] @ K[8].T) * (h[7] != 0))
    dz[6] = rnd((dz[7] @ K[7].T) * (h[6] != 0))
    dz[5] = rnd((dz[6] @ K[6].T) * (h[5] != 0))
    t = dz[5] @ K[5].T
    dz[4] = rnd(t[:, :W] * (h[4] != 0))
    d_enc = t[:, W:]
    for j in (4, 3, 2, 1):
        dz[j - 1] = rnd((dz[j] @ K[j].T) * (h[j - 1] != 0))
    d_enc = d_enc + dz[0] @ K[0].T
    out = torch.zeros(d_enc.shape[0], 64, dtype=torch.float64)
    out[:, :d_enc.shape[1]] = d_enc
    return dict(dz=dz, d_enc=out, dz_out=g)


_ORACLE = {}


def oracle(width):
    """base rows + tail rows of one MLP through the float64 oracle (computed once per width)"""
    if width not in _ORACLE:
        b = make_base(width)
        cond_rows = b['cond'][:, None, :].expand(RAYS, N, 27).reshape(ROWS, 27)
        fwd = forward64(b['params'], b['x'].reshape(ROWS, -1), cond_rows)
        rgb, dens = R.mlp_apply_bf16([[k.double(), bb.double()] for k, bb in b['params']], b['x'].double(), b['cond'].double(),
                                     cfg_of(width))
        fwd['raw_ref'] = torch.cat([rgb.reshape(ROWS, 3), dens.reshape(ROWS, 1)], -1)
        bwd = backward64(b['params'], fwd, b['draw'])
        fwd_t = forward64(b['params'], b['x_tail'].reshape(RAYS, -1), b['cond'])
        bwd_t = backward64(b['params'], fwd_t, b['draw_tail'])
        _ORACLE[width] = dict(base=b, fwd=fwd, bwd=bwd, fwd_tail=fwd_t, bwd_tail=bwd_t)
    return _ORACLE[width]


def conditions(width):
    """what the base rows must satisfy before any GPU comparison means something -> (values, problems)"""
    o = oracle(width)
    raw = torch.cat([o['fwd']['raw'], o['fwd_tail']['raw']])
    d = torch.cdist(raw, raw, p=float('inf'))
    d.fill_diagonal_(float('inf'))
    act = [float((a != 0).double().mean()) for a in o['fwd']['h'] + [o['fwd']['hc']]]
    per_sample = o['fwd']['raw'].reshape(RAYS, N, 4).permute(1, 0, 2)             # [sample, ray, 4]
    ds = torch.cdist(per_sample, per_sample, p=float('inf'))
    ds.diagonal(dim1=1, dim2=2).fill_(float('inf'))
    vals = dict(min_row_distance=float(d.min()), relu_active=act, min_ray_distance_at_a_sample=float(ds.min()))
    bad = []
    if not vals['min_row_distance'] > 0:
        bad.append('two of the %d raw rows are equal' % raw.shape[0])
    if not all(0.1 <= a <= 0.9 for a in act):
        bad.append('ReLU activity outside 10 %% .. 90 %%: %s' % act)
    if not vals['min_ray_distance_at_a_sample'] > 1e-3:
        bad.append('two rays within 1e-3 at a sample: %g' % vals['min_ray_distance_at_a_sample'])
    return vals, bad


# ---------------------------------------------------------------------------------------------------------------------
# the exact-fp32 kernels (csrc/mlp_f32.hip; tests/test_gpu_f32_edges.py): no rounding anywhere, every record compared
# ---------------------------------------------------------------------------------------------------------------------
N24, RAYS24 = 24, 21                    # a second base whose 32-row tiles straddle rays: 504 rows = 15.75 tiles
ROWS24 = N24 * RAYS24
RELU_LAYERS = (0, 1, 2, 3, 4, 5, 6, 7, 10)
DELICATE = 2e-6                         # |pre-activation| below this: the fp32 kernel's own ReLU mask may differ (see delicate_rows)
DELICATE_CAP = 0.02                     # at most this share of a base's rows may be delicate


def f32_spec(width, in_dim):
    """csrc/mlp_f32.hip f32_spec restated: per Dense (fi, fo, x_off, dz_off) in floats of a sample's act / dz record"""
    L, x, d = [], 0, 0
    for l in range(12):
        fi = in_dim if l == 0 else (width + in_dim if l == 5 else (width + 27 if l == 10 else (128 if l == 11 else width)))
        fo = 1 if l == 8 else (128 if l == 10 else (3 if l == 11 else width))
        if l == 9:                      # the bottleneck reads h7 like the density head
            x_off = L[8]['x_off']
        else:
            x_off = x
            x += fi
        L.append(dict(fi=fi, fo=fo, x_off=x_off, dz_off=d))
        d += fo
    return dict(L=L, act=x, dz=d)


def make_params(width, seed):
    """one more MLP of this width, drawn as make_base draws its weights (the objects of a batched call differ) -> params, flat"""
    g = torch.Generator().manual_seed(seed)
    params, flat = [], []
    for fi, fo in R.mlp_layer_shapes(IN_DIM[width], 27, cfg_of(width)):
        lim = (6.0 / (fi + fo)) ** 0.5
        k = (torch.rand(fi, fo, generator=g) * 2 - 1) * lim
        bb = (torch.rand(fo, generator=g) - 0.5) * 0.2
        params.append([k, bb])
        flat += [k.reshape(-1), bb]
    return params, torch.cat(flat)


def make_base24(width):
    """the N = 24 base: make_base's weights and its 16 view directions (ray r looks along cond[r % 16]), encodings and head
    gradients of its own from a second generator, so that make_base's draws stay what they were"""
    b = make_base(width)
    g = torch.Generator().manual_seed(SEEDS[width] + 1000)
    x = torch.randn(RAYS24, N24, b['in_dim'], generator=g).to(torch.bfloat16).float()
    draw = torch.randn(ROWS24, 4, generator=g) * 0.1
    return dict(x=x, cond=b['cond'][torch.arange(RAYS24) % RAYS], draw=draw)


def records64(params, x, cond, draw):
    """x [rows, in_dim], cond [rows, 27], draw [rows, 4] -> everything the fp32 kernels write, in float64 without a rounding:
    raw [rows, 4]; X[l] the INPUT of Dense_l (the act record: x5 = [h4, enc], x8 = x9 = h7, x10 = [bottleneck, view],
    x11 = hc); Z[l] its pre-activation; dz[l] = d(loss)/d Z[l] of all 12 (the dz record: dz11 = d rgb, dz8 = d density, dz9 the
    linear bottleneck's); d_enc [rows, 64]"""
    K = [k.double() for k, _ in params]
    b = [bb.double() for _, bb in params]
    x, cond, g = x.double(), cond.double(), draw.double()
    W = K[1].shape[0]
    X, Z = {}, {}
    h = x
    for l in range(8):
        X[l] = torch.cat([h, x], -1) if l == 5 else h
        Z[l] = X[l] @ K[l] + b[l]
        h = torch.relu(Z[l])
    X[8] = X[9] = h
    Z[8], Z[9] = h @ K[8] + b[8], h @ K[9] + b[9]
    X[10] = torch.cat([Z[9], cond], -1)
    Z[10] = X[10] @ K[10] + b[10]
    X[11] = torch.relu(Z[10])
    Z[11] = X[11] @ K[11] + b[11]
    dz = {11: g[:, :3], 8: g[:, 3:4]}
    dz[10] = (dz[11] @ K[11].T) * (Z[10] > 0)
    dz[9] = dz[10] @ K[10][:W].T
    dz[7] = (dz[9] @ K[9].T + dz[8] @ K[8].T) * (Z[7] > 0)
    dz[6] = (dz[7] @ K[7].T) * (Z[6] > 0)
    dz[5] = (dz[6] @ K[6].T) * (Z[5] > 0)
    t = dz[5] @ K[5].T
    dz[4] = t[:, :W] * (Z[4] > 0)
    for j in (4, 3, 2, 1):
        dz[j - 1] = (dz[j] @ K[j].T) * (Z[j - 1] > 0)
    d_enc = torch.zeros(x.shape[0], 64, dtype=torch.float64)
    d_enc[:, :x.shape[1]] = t[:, W:] + dz[0] @ K[0].T
    return dict(raw=torch.cat([Z[11], Z[8]], -1), X=X, Z=Z, dz=dz, d_enc=d_enc)


def delicate_rows(rec):
    """rows with a ReLU pre-activation within DELICATE of zero.  The fp32 kernels mask the backward by `h > 0` on their OWN
    fp32 record, whose pre-activation differs from float64 by up to 5e-7: there a flipped mask bit is arithmetic, not an error.
    Such rows are left out of the backward comparison with this oracle (never of the forward or a bitwise one).
    -> (bool [rows], smallest |Z| over the ReLU layers, units below 1e-6, units below 1e-5)"""
    za = torch.cat([rec['Z'][l].abs() for l in RELU_LAYERS], -1)
    return (za < DELICATE).any(-1), float(za.min()), int((za < 1e-6).sum()), int((za < 1e-5).sum())


_ORACLE32 = {}


def oracle_f32(width):
    """the three bases of one MLP through records64 (once per width): main 512 rows (N = 32), n24 504 rows, tail 16 rows"""
    if width not in _ORACLE32:
        b, b24 = make_base(width), make_base24(width)
        rows = lambda c, n: c[:, None, :].expand(c.shape[0], n, 27).reshape(-1, 27)
        main = records64(b['params'], b['x'].reshape(ROWS, -1), rows(b['cond'], N), b['draw'])
        n24 = records64(b['params'], b24['x'].reshape(ROWS24, -1), rows(b24['cond'], N24), b24['draw'])
        tail = records64(b['params'], b['x_tail'].reshape(RAYS, -1), b['cond'], b['draw_tail'])
        _ORACLE32[width] = dict(base=b, base24=b24, main=main, n24=n24, tail=tail)
    return _ORACLE32[width]


def conditions_f32(width):
    """-> (values, problems): the delicate rows of every base stay under DELICATE_CAP of its rows, and the N = 24 base is as
    lively as conditions() asks of the N = 32 one"""
    o = oracle_f32(width)
    vals, bad = {}, []
    for name in ('main', 'n24', 'tail'):
        rec = o[name]
        m, zmin, n6, n5 = delicate_rows(rec)
        units = sum(rec['Z'][l].numel() for l in RELU_LAYERS)
        vals[name] = dict(delicate_rows=int(m.sum()), rows=m.numel(), min_abs_z=zmin, units_below_1e6=n6, units_below_1e5=n5,
                          units=units)
        if int(m.sum()) > int(DELICATE_CAP * m.numel()):
            bad.append('%s: %d delicate rows of %d' % (name, int(m.sum()), m.numel()))
    rec = o['n24']
    act = [float((rec['Z'][l] > 0).double().mean()) for l in RELU_LAYERS]
    d = torch.cdist(rec['raw'], rec['raw'], p=float('inf'))
    d.fill_diagonal_(float('inf'))
    vals['n24'].update(relu_active=act, min_row_distance=float(d.min()))
    if not all(0.1 <= a <= 0.9 for a in act):
        bad.append('n24: ReLU activity outside 10 %% .. 90 %%: %s' % act)
    if not float(d.min()) > 0:
        bad.append('n24: two raw rows are equal')
    return vals, bad
