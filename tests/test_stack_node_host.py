"""CPU-side tests of the parameter order the conv-stack node (samplenet_amd/stack_node.py) takes and returns gradients in:
pointnet.stack_param_names / stack_params against each caller's order, kept here as literals -- autograd's returned tuple follows it."""


def test_autoencoder_order_is_the_20_names():
    from samplenet_amd import PointNetAE, pointnet
    from samplenet_amd.autoencoder import _conv_layers

    net = PointNetAE(n_pc_points=64)
    layers = _conv_layers(net)
    assert pointnet.stack_param_names(layers) == [
        "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "conv4.weight", "conv4.bias",
        "conv5.weight", "conv5.bias", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias", "bn3.weight", "bn3.bias", "bn4.weight",
        "bn4.bias", "bn5.weight", "bn5.bias"]
    got = pointnet.stack_params(layers)
    assert len(got) == 20 and all(p is net.get_parameter(n) for p, n in zip(got, pointnet.stack_param_names(layers)))


def test_classifier_order_of_a_two_layer_stack():
    from samplenet_amd import PointNetCls, classifier, pointnet

    net = PointNetCls()
    layers = [classifier._layer(net.transform_net1, "tconv%d" % i, "bn%d" % i, "transform_net1.") for i in (1, 2)]
    names = pointnet.stack_param_names(layers)
    assert names == ["transform_net1.tconv1.weight", "transform_net1.tconv1.bias", "transform_net1.tconv2.weight",
                     "transform_net1.tconv2.bias", "transform_net1.bn1.weight", "transform_net1.bn1.bias", "transform_net1.bn2.weight",
                     "transform_net1.bn2.bias"]
    assert all(p is net.get_parameter(n) for p, n in zip(pointnet.stack_params(layers), names))
    # a layer without BatchNorm (the last FC layer's record) contributes its weight and bias only
    last = pointnet._Layer("fc3", net.fc3, None, None)
    assert pointnet.stack_param_names([last]) == ["fc3.weight", "fc3.bias"] and pointnet.stack_params([last])[1] is net.fc3.bias


def test_set_abstraction_order_has_weights_without_biases_then_the_batchnorm_pairs():
    from samplenet_amd import pointnet, set_abstraction
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    mlp = PM.PointnetSAModule([5, 16, 16], npoint=2, radius=0.5, nsample=4).mlps[0]
    layers = set_abstraction.layer_records(mlp)
    assert all(L.b is None for L in layers)
    names = pointnet.stack_param_names(layers)
    assert names == ["0.conv.weight", "1.conv.weight", "0.bn.weight", "0.bn.bias", "1.bn.weight", "1.bn.bias"]
    assert all(p is mlp.get_parameter(n) for p, n in zip(pointnet.stack_params(layers), names))


def test_sampler_param_order_is_unchanged():
    from samplenet_amd import SampleNet, pointnet

    net = SampleNet(32, 128, 8)
    assert pointnet.param_order(net) == (
        "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "conv4.weight", "conv4.bias",
        "conv5.weight", "conv5.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias", "fc4.weight",
        "fc4.bias", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias", "bn3.weight", "bn3.bias", "bn4.weight", "bn4.bias",
        "bn5.weight", "bn5.bias", "bn_fc1.weight", "bn_fc1.bias", "bn_fc2.weight", "bn_fc2.bias", "bn_fc3.weight", "bn_fc3.bias")
    assert isinstance(pointnet.param_list(net), tuple)
    assert all(p is net.get_parameter(n) for p, n in zip(pointnet.param_list(net), pointnet.param_order(net)))


def test_eval_wgrad_messages_are_the_callers_own():
    from samplenet_amd import classifier, set_abstraction

    assert classifier._WGRAD_NEEDS_TRAINING == (
        "samplenet_amd.classifier: weight gradients need training mode (.train()); an eval-mode network is differentiated "
        "w.r.t. its input only -- freeze it with requires_grad_(False)")
    assert set_abstraction._WGRAD_NEEDS_TRAINING == (
        "samplenet_amd.set_abstraction: weight gradients need training mode (.train()); an eval-mode module is differentiated "
        "w.r.t. its input only -- freeze it with requires_grad_(False)")
