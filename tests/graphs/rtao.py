# Ray-traced ambient occlusion from the raster G-buffer: GBufferRaster's world position and world face
# normal feed RTAO, as in the reference's graphs that show RTAO next to SVAO, in their scripting style.
# The RTAO keys are librsd's optional properties (the reference pass sets them from its GUI); the
# exponential falloff is off here so that the ambient term takes two values only.
# Loaded by tests/test_rtao.py (planned) and tests/test_gpu_rtao.py (executed) with rsd.graph.load_script.
from falcor import *

def render_graph_rtao():
    g = RenderGraph('RTAO')
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    g.create_pass('RTAO', 'RTAO', {'maxTHit': 1.0, 'applyExponentialFalloff': False, 'spp': 1})
    g.add_edge('GBufferRaster.posW', 'RTAO.wPos')
    g.add_edge('GBufferRaster.faceNormalW', 'RTAO.faceNormal')
    g.mark_output('RTAO.ambient')
    g.mark_output('RTAO.rayDistance')
    return g

RTAO = render_graph_rtao()
try: m.addGraph(RTAO)
except NameError: None
