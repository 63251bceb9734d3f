# The dual AO map resolved by the learned net, in the scripting style of the reference's scripts/SAVO_record.py (its
# passes and formulas): SVAO with dualAO writes (bright, dark); ExtractBright / ExtractDark split the pair, ImageEquation1
# makes the importance map, the linear depth is divided by 1000; the four images are split into 16 quarter-size layers,
# ConvolutionalNet resolves them, InterleaveTexture puts the AO back together and ImageEquation shows it as grey.
# Loaded by tests/test_gpu_graph_convnet.py with rsd.graph.load_script, the weights placeholder replaced by a directory the test
# writes with rsd.convnet.save_dir.
from falcor import *

def render_graph_svao_convnet():
    g = RenderGraph('SVAOConvNet')
    g.create_pass('GuardBand', 'GuardBand', {'guardBand': 8})
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    g.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('CompressNormals', 'CompressNormals', {'viewSpace': True, 'use16Bit': True})
    g.create_pass('SVAO', 'SVAO', {'radius': 1.0, 'primaryDepthMode': 'SingleDepth', 'secondaryDepthMode': 'StochasticDepth', 'exponent': 2.0, 'thickness': 0.0, 'stochMapDivisor': 2, 'dualAO': True, 'alphaTest': True, 'stochGuardBand': 64})
    g.create_pass('ExtractBright', 'ImageEquation', {'formula': 'I0[xy].xxxx', 'format': 'R8Unorm'})
    g.create_pass('ExtractDark', 'ImageEquation', {'formula': 'I0[xy].gggg', 'format': 'R8Unorm'})
    g.create_pass('ImageEquation1', 'ImageEquation', {'formula': '1.0 - max(I0[xy].x-I0[xy].y, 0.05)', 'format': 'R8Unorm'})
    g.create_pass('ImageEquationLinearDepth', 'ImageEquation', {'formula': 'I0[xy]/1000.0', 'format': 'R32Float'})
    g.create_pass('DeinterleaveBright', 'DeinterleaveTexture', {})
    g.create_pass('DeinterleaveDark', 'DeinterleaveTexture', {})
    g.create_pass('DeinterleaveTexture', 'DeinterleaveTexture', {})
    g.create_pass('DeinterleaveDepth', 'DeinterleaveTexture', {})
    g.create_pass('ConvolutionalNet', 'ConvolutionalNet', {'weights': 'WEIGHTS_DIR', 'numerics': 'Exact'})
    g.create_pass('InterleaveTexture', 'InterleaveTexture', {})
    g.create_pass('AmbientNet', 'ImageEquation', {'formula': 'I0[xy].rrra', 'format': 'RGBA32Float'})
    g.add_edge('GuardBand', 'GBufferRaster')
    g.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')
    g.add_edge('GBufferRaster.faceNormalW', 'CompressNormals.normalW')
    g.add_edge('LinearizeDepth.linearDepth', 'SVAO.depth')
    g.add_edge('CompressNormals.normalOut', 'SVAO.normals')
    g.add_edge('SVAO.ao', 'ExtractBright.I0')
    g.add_edge('SVAO.ao', 'ExtractDark.I0')
    g.add_edge('SVAO.ao', 'ImageEquation1.I0')
    g.add_edge('LinearizeDepth.linearDepth', 'ImageEquationLinearDepth.I0')
    g.add_edge('ExtractBright.out', 'DeinterleaveBright.texIn')
    g.add_edge('ExtractDark.out', 'DeinterleaveDark.texIn')
    g.add_edge('ImageEquation1.out', 'DeinterleaveTexture.texIn')
    g.add_edge('ImageEquationLinearDepth.out', 'DeinterleaveDepth.texIn')
    g.add_edge('DeinterleaveBright.texOut', 'ConvolutionalNet.bright')
    g.add_edge('DeinterleaveDark.texOut', 'ConvolutionalNet.dark')
    g.add_edge('DeinterleaveTexture.texOut', 'ConvolutionalNet.importance')
    g.add_edge('DeinterleaveDepth.texOut', 'ConvolutionalNet.depth')
    g.add_edge('ConvolutionalNet.out', 'InterleaveTexture.texIn')
    g.add_edge('InterleaveTexture.texOut', 'AmbientNet.I0')
    g.mark_output('SVAO.ao')
    g.mark_output('DeinterleaveBright.texOut')
    g.mark_output('DeinterleaveDark.texOut')
    g.mark_output('DeinterleaveTexture.texOut')
    g.mark_output('DeinterleaveDepth.texOut')
    g.mark_output('ImageEquation1.out')
    g.mark_output('ImageEquationLinearDepth.out')
    g.mark_output('ConvolutionalNet.out')
    g.mark_output('InterleaveTexture.texOut')
    g.mark_output('AmbientNet.out')
    return g

SVAOConvNet = render_graph_svao_convnet()
try: m.addGraph(SVAOConvNet)
except NameError: None
