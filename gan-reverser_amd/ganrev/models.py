"""Mirror of the reference model zoo's live constructors (models.lua): create_G -> create_G3 (models.lua:201-203,
104-143), create_R -> create_R_default (models.lua:385-387, 389-464) and create_D -> create_D2 (models.lua:209-211, 272-337;
the discriminator adversarial.lua trains G against - SURVEY.md 8f rank 4); create_G_encoder (models.lua:57-102, pretrain_g.lua's
encoder half) and the two D variants with average pooling, create_D_default and create_D_facegen (models.lua:213-270, 339-383),
which nothing selects (the reference's create_D returns create_D2); create_G4 (models.lua:145-194), the 32-branch generator
that nothing selects either; createResidual (models.lua:8-55), the residual block the
reference's author left for edited models.  Same layer lists, same argument meaning."""
from . import nn
from .weight_init import w_init


class _CudnnSpatialConvolution(nn.SpatialConvolution):
    TYPENAME = "cudnn.SpatialConvolution"      # not matched by weight-init.lua:54 (only the bias is zeroed)


class _CudnnReLU(nn.ReLU):
    TYPENAME = "cudnn.ReLU"


def createResidual(nbInputPlanes, nbInnerPlanes, nbOutputPlanes, activation=None, bn=True):
    """models.lua:8-55: [1x1 in -> inner] - 3x3 - 3x3 - [1x1 inner -> out], each followed by [BatchNorm and] the activation, summed with
    the shortcut: the input itself when in = out, else a 1x1 reducer with [BatchNorm and] the activation.  The bracketed 1x1 layers
    exist only where the plane counts differ.  No seed and no w_init: the reference's function has neither."""
    if activation is None or activation == "ReLU":
        def act(): return _CudnnReLU(True)
    elif activation == "PReLU":
        def act(): return nn.PReLU()
    elif activation == "LeakyReLU":
        def act(): return nn.LeakyReLU(0.333)
    else:
        raise ValueError("Unknown activation '%s'" % (activation,))
    assert bn is True or bn is False

    def block(seq, nin, nout, k):
        seq.add(_CudnnSpatialConvolution(nin, nout, k, k, 1, 1, k // 2, k // 2))
        if bn:
            seq.add(nn.SpatialBatchNormalization(nout))
        seq.add(act())

    seq = nn.Sequential()
    inner = nn.Sequential()
    if nbInputPlanes != nbInnerPlanes:
        block(inner, nbInputPlanes, nbInnerPlanes, 1)
    block(inner, nbInnerPlanes, nbInnerPlanes, 3)
    block(inner, nbInnerPlanes, nbInnerPlanes, 3)
    if nbInnerPlanes != nbOutputPlanes:
        block(inner, nbInnerPlanes, nbOutputPlanes, 1)
    conc = nn.ConcatTable(2)
    conc.add(inner)
    if nbInputPlanes == nbOutputPlanes:
        conc.add(nn.Identity())
    else:
        reducer = nn.Sequential()
        block(reducer, nbInputPlanes, nbOutputPlanes, 1)
        conc.add(reducer)
    seq.add(conc)
    seq.add(nn.CAddTable())
    return seq


def create_G3(dimensions, noiseDim, cuda=True, seed=0):
    """models.lua:104-143.  dimensions = (channels, height, width)."""
    nn.manualSeed(seed)          # the cudnn.* convolutions and the BatchNorm gammas keep their constructor draw (weight-init.lua:54-67)
    model = nn.Sequential()
    if cuda:
        model.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    startHeight = dimensions[1] // 2 // 2
    startWidth = dimensions[2] // 2 // 2
    model.add(nn.Linear(noiseDim, 512 * startHeight * startWidth))
    model.add(nn.BatchNormalization(512 * startHeight * startWidth))
    model.add(_CudnnReLU(True))
    model.add(nn.View(512, startHeight, startWidth))
    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(_CudnnSpatialConvolution(512, 256, 3, 3, 1, 1, 1, 1))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(_CudnnReLU(True))
    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(_CudnnSpatialConvolution(256, 128, 3, 3, 1, 1, 1, 1))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(_CudnnReLU(True))
    model.add(_CudnnSpatialConvolution(128, dimensions[0], 3, 3, 1, 1, 1, 1))
    model.add(nn.Sigmoid())
    if cuda:
        model.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        model.cuda()
    return w_init(model, "heuristic", seed)


def create_G4(dimensions, noiseDim, cuda=True, seed=0):
    """models.lua:145-194: nn.Concat(2) of 32 branches, each Linear(noiseDim, 16) - PReLU - Linear(16, 16*16*16) - BatchNorm - PReLU -
    Reshape(16, 16, 16) - up-sampling - 3x3 conv 16 -> 16 - BatchNorm - PReLU, joined to 512 x 32 x 32; then a 3x3 conv 512 -> 64 -
    BatchNorm - PReLU and a 3x3 conv 64 -> channels - Sigmoid.  As in the reference, startHeight / startWidth are computed and not
    used: the branches are 16 x 16 whatever `dimensions` says, so the output is channels x 32 x 32.  The 32 branches are
    structurally identical, so the model compiles to ONE grouped gr_net (nn.bundle_plan) and is a plain net to every caller."""
    nn.manualSeed(seed)
    model = nn.Sequential()
    if cuda:
        model.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    startHeight = dimensions[1] // 2 // 2          # models.lua:152-153: computed, used nowhere
    startWidth = dimensions[2] // 2 // 2
    concat = nn.Concat(2)
    for _ in range(32):
        seq = nn.Sequential()
        seq.add(nn.Linear(noiseDim, 16))
        seq.add(nn.PReLU())
        seq.add(nn.Linear(16, 16 * 16 * 16))
        seq.add(nn.BatchNormalization(16 * 16 * 16))
        seq.add(nn.PReLU())
        seq.add(nn.Reshape(16, 16, 16))
        seq.add(nn.SpatialUpSamplingNearest(2))
        seq.add(_CudnnSpatialConvolution(16, 16, 3, 3, 1, 1, 1, 1))
        seq.add(nn.SpatialBatchNormalization(16))
        seq.add(nn.PReLU())
        concat.add(seq)
    model.add(concat)
    model.add(_CudnnSpatialConvolution(32 * 16, 64, 3, 3, 1, 1, 1, 1))
    model.add(nn.SpatialBatchNormalization(64))
    model.add(nn.PReLU())
    model.add(_CudnnSpatialConvolution(64, dimensions[0], 3, 3, 1, 1, 1, 1))
    model.add(nn.Sigmoid())
    if cuda:
        model.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        model.cuda()
    return w_init(model, "heuristic", seed)     # top-level modules only: the two tail convolutions get their bias zeroed, no branch is touched


def create_G_encoder(dimensions, noiseDim, cuda=True, seed=0):
    """models.lua:57-102: three 3x3 conv - BatchNorm - ReLU blocks, halved by an average pool and two max pools, then
    Linear - BatchNorm - ReLU - Linear - Tanh down to noiseDim.  Built from cudnn.* like create_G3: the heuristic init only
    zeroes the convolutions' biases (weight-init.lua:54-72)."""
    nn.manualSeed(seed)
    model = nn.Sequential()
    if cuda:
        model.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    startHeight, startWidth = dimensions[1], dimensions[2]
    model.add(_CudnnSpatialConvolution(dimensions[0], 16, 3, 3, 1, 1, 1, 1))     # 32x32 -> 16x16  (models.lua:68-71)
    model.add(nn.SpatialBatchNormalization(16))
    model.add(_CudnnReLU(True))
    model.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    model.add(_CudnnSpatialConvolution(16, 32, 3, 3, 1, 1, 1, 1))                # 16x16 -> 8x8  (models.lua:74-77)
    model.add(nn.SpatialBatchNormalization(32))
    model.add(_CudnnReLU(True))
    model.add(nn.SpatialMaxPooling(2, 2))
    model.add(_CudnnSpatialConvolution(32, 64, 3, 3, 1, 1, 1, 1))                # 8x8 -> 4x4  (models.lua:80-83)
    model.add(nn.SpatialBatchNormalization(64))
    model.add(_CudnnReLU(True))
    model.add(nn.SpatialMaxPooling(2, 2))
    height, width = startHeight // 2 // 2 // 2, startWidth // 2 // 2 // 2
    model.add(nn.View(64 * height * width))
    model.add(nn.Linear(64 * height * width, 512))
    model.add(nn.BatchNormalization(512))
    model.add(_CudnnReLU(True))
    model.add(nn.Linear(512, noiseDim))
    model.add(nn.Tanh())
    if cuda:
        model.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        model.cuda()
    return w_init(model, "heuristic", seed)


def create_VAE_encoder(dimensions, noiseDim, cuda=True, seed=0):
    """The reference has no counterpart: models.lua holds no variational model (its README only asks to compare with one).  This is
    create_G_encoder's trunk, unchanged, under the head a VAE needs: nn.Linear(512, 2 noiseDim) with no
    nn.Tanh behind it - columns 0 .. noiseDim - 1 of the output are the mean, the rest the log-variance (ganrev.vae, gr_vae_sample_dev)."""
    model = create_G_encoder(dimensions, 2 * noiseDim, cuda, seed)
    model.modules = [m for m in model.modules if not isinstance(m, nn.Tanh)]
    return model


def create_G(dimensions, noiseDim, cuda=True, seed=0):
    return create_G3(dimensions, noiseDim, cuda, seed)        # models.lua:201-203


def create_R_default(dimensions, noiseDim, noiseMethod="normal", fixer=False, cuda=True, seed=0):
    """models.lua:389-464."""
    assert noiseMethod in ("normal", "uniform")                # models.lua:390
    nn.manualSeed(seed)
    conv = nn.Sequential()
    if cuda:
        conv.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    if fixer:
        conv.add(nn.Dropout(0.5, True).keepAlwaysOn())         # models.lua:399-406
    c = dimensions[0]
    for block, (cin, cout) in enumerate([(c, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128)]):
        conv.add(nn.SpatialConvolution(cin, cout, 3, 3, 1, 1, 1, 1))
        conv.add(nn.SpatialBatchNormalization(cout))
        conv.add(nn.ELU())
        if block == 2:                                          # models.lua:419-423
            conv.add(nn.SpatialMaxPooling(2, 2))
            conv.add(nn.Dropout())
        elif block == 5:                                        # models.lua:436-440
            conv.add(nn.SpatialDropout(0.25))
            conv.add(nn.SpatialMaxPooling(2, 2))
        else:
            conv.add(nn.Dropout())
    height = dimensions[1] // 2 // 2
    width = dimensions[2] // 2 // 2
    conv.add(nn.View(128 * height * width))
    conv.add(nn.Linear(128 * height * width, 512))
    conv.add(nn.BatchNormalization(512))
    conv.add(nn.ELU())
    conv.add(nn.Dropout(0.5))
    conv.add(nn.Linear(512, noiseDim))
    if noiseMethod != "normal":
        conv.add(nn.Tanh())
    if cuda:
        conv.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        conv.cuda()
    return w_init(conv, "heuristic", seed)


def create_R(dimensions, noiseDim, noiseMethod="normal", fixer=False, cuda=True, seed=0):
    return create_R_default(dimensions, noiseDim, noiseMethod, fixer, cuda, seed)   # models.lua:385-387


def create_D2(dimensions, cuda=True, seed=0):
    """models.lua:272-337: two 3x3 convolutions, then nn.Concat(2) of a 5x5 tower and a deeper 3x3 tower, joined by two Linear
    layers into one sigmoid unit.  Every activation is an nn.PReLU() with its own learnable slope."""
    nn.manualSeed(seed)

    def createNxN(nbKernelsIn, nbKernelsOut, kernelSize, dropout):      # models.lua:273-281
        model = nn.Sequential()
        pad = (kernelSize - 1) // 2
        model.add(nn.SpatialConvolution(nbKernelsIn, nbKernelsOut, kernelSize, kernelSize, 1, 1, pad, pad))
        model.add(nn.PReLU())
        if dropout > 0:
            model.add(nn.SpatialDropout(0.25))
        return model

    conv = nn.Sequential()
    if cuda:
        conv.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    conv.add(createNxN(dimensions[0], 128, 3, 0))
    conv.add(createNxN(128, 128, 3, 0.2))
    conv.add(nn.SpatialMaxPooling(2, 2))
    concat = nn.Concat(2)
    left, right = nn.Sequential(), nn.Sequential()
    h4, w4 = dimensions[1] // 2 // 2, dimensions[2] // 2 // 2
    left.add(createNxN(128, 64, 5, 0.2))
    left.add(nn.SpatialMaxPooling(2, 2))
    left.add(nn.View(64 * h4 * w4))
    left.add(nn.Linear(64 * h4 * w4, 512))
    left.add(nn.PReLU())
    left.add(nn.Dropout(0.25))
    right.add(createNxN(128, 128, 3, 0.2))
    right.add(nn.SpatialMaxPooling(2, 2))
    right.add(createNxN(128, 256, 3, 0.2))
    right.add(createNxN(256, 256, 3, 0.2))
    right.add(nn.SpatialMaxPooling(2, 2))
    height, width = dimensions[1] // 2 // 2 // 2, dimensions[2] // 2 // 2 // 2
    right.add(nn.View(256 * height * width))
    right.add(nn.Linear(256 * height * width, 512))
    right.add(nn.PReLU())
    concat.add(left)
    concat.add(right)
    conv.add(concat)
    conv.add(nn.Linear(512 + 512, 256))
    conv.add(nn.PReLU())
    conv.add(nn.Dropout(0.25))
    conv.add(nn.Linear(256, 1))
    conv.add(nn.Sigmoid())
    if cuda:
        conv.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        conv.cuda()
    return w_init(conv, "heuristic", seed)


def create_D_default(dimensions, cuda=True, seed=0):
    """models.lua:213-270: five 3x3 convolutions, each closed by a PReLU (one slope); SpatialDropout(0.25) behind all but the
    first, a 2x2 average pool behind the last three; Linear - PReLU - Dropout(0.5) - Linear - Sigmoid."""
    nn.manualSeed(seed)
    conv = nn.Sequential()
    if cuda:
        conv.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    for cin, cout, drop, pool in [(dimensions[0], 32, False, False), (32, 64, True, False), (64, 128, True, True),
                                  (128, 256, True, True), (256, 512, True, True)]:
        conv.add(nn.SpatialConvolution(cin, cout, 3, 3, 1, 1, 1, 1))
        conv.add(nn.PReLU())
        if drop:
            conv.add(nn.SpatialDropout(0.25))
        if pool:
            conv.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    height, width = dimensions[1] // 2 // 2 // 2, dimensions[2] // 2 // 2 // 2
    conv.add(nn.View(512 * height * width))
    conv.add(nn.Linear(512 * height * width, 512))
    conv.add(nn.PReLU())
    conv.add(nn.Dropout(0.5))
    conv.add(nn.Linear(512, 1))
    conv.add(nn.Sigmoid())
    if cuda:
        conv.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        conv.cuda()
    return w_init(conv, "heuristic", seed)


def create_D_facegen(dimensions, cuda=True, seed=0):
    """models.lua:339-383: four conv - PReLU - SpatialDropout(0.2) - average-pool blocks (SpatialConvolution(a, b, 3, 3, 1, 1, 1):
    padH defaults to padW), then Linear - PReLU - Dropout() twice and Linear - Sigmoid.  nn.PReLU(nil, nil, true) is the
    one-slope PReLU (nn.PReLU takes only nOutputPlane); nn.Dropout() is p = 0.5."""
    nn.manualSeed(seed)
    conv = nn.Sequential()
    if cuda:
        conv.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    for cin, cout in [(dimensions[0], 64), (64, 128), (128, 256), (256, 512)]:
        conv.add(nn.SpatialConvolution(cin, cout, 3, 3, 1, 1, 1))
        conv.add(nn.PReLU())
        conv.add(nn.SpatialDropout(0.2))
        conv.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    flat = 512 * (dimensions[1] // 16) * (dimensions[2] // 16)           # 512 * 0.25^4 * height * width
    conv.add(nn.View(flat))
    conv.add(nn.Linear(flat, 512))
    conv.add(nn.PReLU())
    conv.add(nn.Dropout())
    conv.add(nn.Linear(512, 512))
    conv.add(nn.PReLU())
    conv.add(nn.Dropout())
    conv.add(nn.Linear(512, 1))
    conv.add(nn.Sigmoid())
    if cuda:
        conv.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        conv.cuda()
    return w_init(conv, "heuristic", seed)


def create_D(dimensions, cuda=True, seed=0):
    return create_D2(dimensions, cuda, seed)                           # models.lua:209-211
