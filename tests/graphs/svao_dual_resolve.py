# The dual AO map resolved into one AO value, in the scripting style of the reference's scripts/SVAO_depth.py:
#   SVAODualResolve  SVAO with dualAO writes (bright, dark); the map and the linear depth are split into 16
#                    quarter-size layers, AOGuidedBlur resolves them, InterleaveTexture puts the AO back together,
#                    CrossBilateralBlur smooths it and ImageEquation shows it as grey;
#   HBAOResolve      HBAO's ambientMap is 16 RG8Unorm layers already and feeds AOGuidedBlur directly.
# Loaded by tests/test_ao_resolve.py (planned) and tests/test_gpu_graph_ao_resolve.py (executed, with 'enabled'
# replaced for one case) with rsd.graph.load_script.
from falcor import *

def render_graph_svao_dual_resolve():
    g = RenderGraph('SVAODualResolve')
    g.create_pass('GuardBand', 'GuardBand', {'guardBand': 16})
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    g.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('CompressNormals', 'CompressNormals', {'viewSpace': True, 'use16Bit': True})
    g.create_pass('SVAO', 'SVAO', {'radius': 1.0, 'primaryDepthMode': 'SingleDepth', 'secondaryDepthMode': 'StochasticDepth', 'exponent': 2.0, 'thickness': 0.0, 'stochMapDivisor': 2, 'dualAO': True, 'alphaTest': True, 'stochGuardBand': 64})
    g.create_pass('DeinterleaveBrightDark', 'DeinterleaveTexture', {})
    g.create_pass('DeinterleaveDepth', 'DeinterleaveTexture', {})
    g.create_pass('AOGuidedBlur', 'AOGuidedBlur', {'kernelRadius': 2, 'clampResults': True, 'enabled': True})
    g.create_pass('InterleaveTexture0', 'InterleaveTexture', {})
    g.create_pass('CrossBilateralBlurBL', 'CrossBilateralBlur', {})
    g.create_pass('Ambient', 'ImageEquation', {'formula': 'I0[xy].rrra', 'format': 'RGBA32Float'})
    g.add_edge('GuardBand', 'GBufferRaster')
    g.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')
    g.add_edge('GBufferRaster.faceNormalW', 'CompressNormals.normalW')
    g.add_edge('LinearizeDepth.linearDepth', 'SVAO.depth')
    g.add_edge('CompressNormals.normalOut', 'SVAO.normals')
    g.add_edge('SVAO.ao', 'DeinterleaveBrightDark.texIn')
    g.add_edge('LinearizeDepth.linearDepth', 'DeinterleaveDepth.texIn')
    g.add_edge('DeinterleaveBrightDark.texOut', 'AOGuidedBlur.ao2')
    g.add_edge('DeinterleaveDepth.texOut', 'AOGuidedBlur.lineardepth')
    g.add_edge('AOGuidedBlur.color', 'InterleaveTexture0.texIn')
    g.add_edge('InterleaveTexture0.texOut', 'CrossBilateralBlurBL.color')
    g.add_edge('LinearizeDepth.linearDepth', 'CrossBilateralBlurBL.linear depth')
    g.add_edge('CrossBilateralBlurBL.colorOut', 'Ambient.I0')
    g.mark_output('SVAO.ao')
    g.mark_output('LinearizeDepth.linearDepth')
    g.mark_output('AOGuidedBlur.color')
    g.mark_output('Ambient.out')
    return g

def render_graph_hbao_resolve():
    h = RenderGraph('HBAOResolve')
    h.create_pass('GuardBand', 'GuardBand', {'guardBand': 16})
    h.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    h.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    h.create_pass('DeinterleaveDepth', 'DeinterleaveTexture', {})
    h.create_pass('HBAO', 'HBAO', {'radius': 1.0, 'depthMode': 'SingleDepth', 'depthBias': 0.1, 'exponent': 2.0})
    h.create_pass('AOGuidedBlur', 'AOGuidedBlur', {'kernelRadius': 4, 'clampResults': True, 'enabled': True, 'localDeviation': False})
    h.create_pass('InterleaveAO', 'InterleaveTexture', {})
    h.add_edge('GuardBand', 'GBufferRaster')
    h.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    h.add_edge('LinearizeDepth.linearDepth', 'DeinterleaveDepth.texIn')
    h.add_edge('DeinterleaveDepth.texOut', 'HBAO.depth')
    h.add_edge('GBufferRaster.faceNormalW', 'HBAO.normals')
    h.add_edge('HBAO.ambientMap', 'AOGuidedBlur.ao2')
    h.add_edge('DeinterleaveDepth.texOut', 'AOGuidedBlur.lineardepth')
    h.add_edge('AOGuidedBlur.color', 'InterleaveAO.texIn')
    h.mark_output('HBAO.ambientMap')
    h.mark_output('DeinterleaveDepth.texOut')
    h.mark_output('AOGuidedBlur.color')
    h.mark_output('InterleaveAO.texOut')
    return h

SVAODualResolve = render_graph_svao_dual_resolve()
HBAOResolve = render_graph_hbao_resolve()
try:
    m.addGraph(SVAODualResolve)
    m.addGraph(HBAOResolve)
except NameError: None
