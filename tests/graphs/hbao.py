# Deinterleaved horizon-based AO as a graph: the linear depth and a peeled, linearised second layer are split
# into 16 quarter-size layers each, HBAO shades them, InterleaveTexture puts the (bright, dark) map back together,
# CrossBilateralBlur blurs its bright channel and ImageEquation shows it as grey.  Loaded by tests/test_hbao.py
# (planned) and tests/test_gpu_hbao.py (executed, with 'depthMode' replaced per test) with rsd.graph.load_script.
from falcor import *

def render_graph_hbao():
    g = RenderGraph('HBAOGraph')
    g.create_pass('GuardBand', 'GuardBand', {'guardBand': 16})
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    g.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('DepthPeeling', 'DepthPeeling', {'cullMode': 'Back', 'depthFormat': 'D32Float', 'minSeparationDistance': 0.5})
    g.create_pass('LinearizeDepth2', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('DeinterleaveDepth', 'DeinterleaveTexture', {})
    g.create_pass('DeinterleaveDepth2', 'DeinterleaveTexture', {})
    g.create_pass('HBAO', 'HBAO', {'radius': 1.0, 'depthMode': 'DualDepth', 'depthBias': 0.1, 'exponent': 2.0})
    g.create_pass('InterleaveAO', 'InterleaveTexture', {})
    g.create_pass('BlurAO', 'CrossBilateralBlur', {})
    g.create_pass('Ambient', 'ImageEquation', {'formula': 'I0[xy].rrra', 'format': 'RGBA32Float'})
    g.add_edge('GuardBand', 'GBufferRaster')
    g.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    g.add_edge('LinearizeDepth.linearDepth', 'DepthPeeling.linearZ')
    g.add_edge('DepthPeeling.depth2', 'LinearizeDepth2.depth')
    g.add_edge('LinearizeDepth.linearDepth', 'DeinterleaveDepth.texIn')
    g.add_edge('LinearizeDepth2.linearDepth', 'DeinterleaveDepth2.texIn')
    g.add_edge('DeinterleaveDepth.texOut', 'HBAO.depth')
    g.add_edge('DeinterleaveDepth2.texOut', 'HBAO.depth2')
    g.add_edge('GBufferRaster.faceNormalW', 'HBAO.normals')
    g.add_edge('HBAO.ambientMap', 'InterleaveAO.texIn')
    g.add_edge('InterleaveAO.texOut', 'BlurAO.color')
    g.add_edge('LinearizeDepth.linearDepth', 'BlurAO.linear depth')
    g.add_edge('BlurAO.colorOut', 'Ambient.I0')
    g.mark_output('HBAO.ambientMap')
    g.mark_output('Ambient.out')
    return g

HBAOGraph = render_graph_hbao()
try: m.addGraph(HBAOGraph)
except NameError: None
