"""ResNet-18 variant of the reference (sheep/resnet.py:6-160), MI355X-native.

Same class names, constructor arguments, attribute names and parameter paths
(``conv1``, ``bn1``, ``res2`` ... ``res5``; per block ``conv1/bn1/conv2/bn2``
and the strided 3x3 ``conv3/bn3`` shortcut of ``BasicA``), so snapshots
interchange.  Each block's ``__call__`` is one fused function node
(functions/blocks.py).  Only the basic-block depths the LoANs trainer can
instantiate (18 / 20 / 34) are built; the bottleneck variants
(sheep/resnet.py:163-216) belong to the ResNet-50 localizer.
``class_labels=K`` adds the ImageNet head of sheep/resnet.py:65-87: global average pooling and ``fc = L.Linear(None, K)``.
"""
from .. import links as L
from ..functions import blocks, drop_path, global_average_pooling_2d, linear
from ..runtime.core import Chain, ChainList


class ResNet(Chain, drop_path.DropPathOwner):

    def __init__(self, n_layers, class_labels=None):
        super(ResNet, self).__init__()
        w = L.HeNormal()
        if n_layers == 18:
            block = [2, 2, 2, 2]
        elif n_layers == 20:
            block = [2, 2, 2, 2, 2, 2]
        elif n_layers == 34:
            block = [3, 4, 6, 3]
        else:
            raise ValueError("You tried to create a ResNet variant that does not exist")
        with self.init_scope():
            self.conv1 = L.Convolution2D(3, 64, 7, 2, 3, initialW=w, dense_rows=True)
            self.bn1 = L.BatchNormalization(64)
            self.res2 = BasicBlock(block[0], 64, 1, in_ch=64)
            self.res3 = BasicBlock(block[1], 128, in_ch=64)
            self.res4 = BasicBlock(block[2], 256, in_ch=128)
            self.res5 = BasicBlock(block[3], 512, in_ch=256)
            if n_layers == 20:
                self.res6 = BasicBlock(block[4], 512, in_ch=512)
                self.res7 = BasicBlock(block[5], 512, in_ch=512)
            if class_labels is not None:
                self.fc = L.Linear(None, class_labels)      # Chainer's default initialiser: LeCunNormal, zero bias

        self.n_layers = n_layers
        self.class_labels = class_labels

    # data parallel: the gradient arena is exchanged in three parts, cut in front of these stages -- everything from res5 up
    # (res5 + the head + res6 / res7: 75 % of the bytes at 224 px) as soon as the backward has left res5, res4 (19 %) next,
    # the rest when the backward ends (loans_amd/parallel.py)
    exchange_stages = ('res4', 'res5')

    def materialize_head(self):
        """Size the lazily sized ``fc`` (the last stage has 512 channels at every depth).  A parameter can only join the
        model's arena before ``finalize``, so whoever finalises the tree (the localizer, ``Classifier``) calls this first."""
        if self.class_labels is not None:
            self.fc.ensure_initialized(512)

    def drop_path_stages(self):
        """the stages whose residual units ``set_drop_path`` counts, in forward order"""
        return [getattr(self, n) for n in ('res2', 'res3', 'res4', 'res5', 'res6', 'res7') if hasattr(self, n)]

    def __call__(self, x):
        """x: preprocessed frames (``prepare_images``: the padded packed-RGB buffer conv1 reads).  Returns the NHWC feature map,
        or the (B, class_labels) logits when the model has the classification head."""
        self.materialize_head()
        self.draw_drop_path(x.shape[0], x.data.device)      # stochastic depth: one keep table per training forward
        h = blocks.StemFunction(self.conv1, self.bn1)(x, self.conv1.W, self.conv1.b, self.bn1.gamma, self.bn1.beta)
        h = self.res2(h)
        h = self.res3(h)
        h = self.res4(blocks.stage_boundary(self, 'res4', h))
        if hasattr(self, 'res5'):
            h = self.res5(blocks.stage_boundary(self, 'res5', h))
        if hasattr(self, 'res6'):
            h = self.res6(h)
        if hasattr(self, 'res7'):
            h = self.res7(h)
        if self.class_labels is not None:
            h = global_average_pooling_2d(h)        # average_pooling_2d(h, (H, W), stride=1)
            h = linear(h, self.fc.W, self.fc.b)
        return h


class BasicBlock(ChainList):

    def __init__(self, layer, ch, stride=2, in_ch=None):
        super(BasicBlock, self).__init__()
        in_ch = ch if in_ch is None else in_ch      # the reference infers it lazily (Convolution2D(None, ...))
        self.add_link(BasicA(ch, stride, in_ch))
        for i in range(layer - 1):
            self.add_link(BasicB(ch))

    def __call__(self, x):
        for f in self.children():
            x = f(x)
        return x


class BasicA(Chain):

    def __init__(self, ch, stride, in_ch=None):
        super(BasicA, self).__init__()
        w = L.HeNormal()
        in_ch = ch if in_ch is None else in_ch
        with self.init_scope():
            self.conv1 = L.Convolution2D(in_ch, ch, 3, stride, 1, initialW=w, nobias=True)
            self.bn1 = L.BatchNormalization(ch)
            self.conv2 = L.Convolution2D(ch, ch, 3, 1, 1, initialW=w, nobias=True)
            self.bn2 = L.BatchNormalization(ch)

            self.conv3 = L.Convolution2D(in_ch, ch, 3, stride, 1, initialW=w, nobias=True)
            self.bn3 = L.BatchNormalization(ch)

    def __call__(self, x):
        return blocks.residual_unit(x, [(self.conv1, self.bn1), (self.conv2, self.bn2)], (self.conv3, self.bn3),
                                    drop=drop_path.unit_vector(self))


class BasicB(Chain):

    def __init__(self, ch):
        super(BasicB, self).__init__()
        w = L.HeNormal()
        with self.init_scope():
            self.conv1 = L.Convolution2D(ch, ch, 3, 1, 1, initialW=w, nobias=True)
            self.bn1 = L.BatchNormalization(ch)
            self.conv2 = L.Convolution2D(ch, ch, 3, 1, 1, initialW=w, nobias=True)
            self.bn2 = L.BatchNormalization(ch)

    def __call__(self, x):
        return blocks.residual_unit(x, [(self.conv1, self.bn1), (self.conv2, self.bn2)], drop=drop_path.unit_vector(self))
